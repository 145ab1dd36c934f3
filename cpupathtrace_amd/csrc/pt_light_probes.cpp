// pt_light_probes.cpp -- the entry points of include/pt_light_probes.h: SH radiance at free points, at the nodes of a grid,
// and the lookup that shades points from a grid's records.  The kernels are pt_light_probe_kernels.h's (in pt_walks.hip); this unit checks
// the arguments, keeps the workspace -- one per device, grown on demand, as the denoiser keeps its own (pt_image.cpp); pt_scene is as it
// was -- and cuts a call into launches of whole probes: at most PT_LIGHT_PROBE_CHUNK (probe, sample) pairs each, read per call.  A
// sample's engine is seeded with its probe's index in the call, and a probe's record is reduced in an order of its own, so the cut changes no bit.  Nothing here changes the scene, so every call is allowed
// with a live pt_frame and with or without a motion mark.
#include "pt_host.h"

#include <cmath>

using namespace pth;

namespace {

const uint64_t LIGHT_PROBE_MAX = 0x7fffffffULL;
const int LIGHT_PROBE_CHUNK_DEFAULT = 2 << 20;

// The buffers of the calls on one device: the host forms' positions, records, points and values, and the workspace of one launch -- two
// float4 per (probe, sample) pair and the walks' spill area.  One call at a time per device (`mutex`, taken behind the scene's render lock);
// `last` marks the end of the latest device-form call, whose work may still run when the next call comes: that call waits for it before
// it touches a buffer.  Lives as long as the process (never freed: a static destructor would run after the HIP runtime has gone).
struct LightProbeWorkspace {
    std::mutex mutex;
    DevBuf<float> positions;
    DevBuf<pt_light_probe> out;
    DevBuf<F4> plane;
    DevBuf<uint2> spill;
    DevBuf<float> points;
    DevBuf<F4> values;
    hipEvent_t last = nullptr;
    bool pending = false;
};

LightProbeWorkspace &workspace(int device) {
    static std::mutex table_mutex;
    static std::vector<LightProbeWorkspace *> table;
    std::lock_guard<std::mutex> lock(table_mutex);
    if(static_cast<size_t>(device) >= table.size()) {
        table.resize(static_cast<size_t>(device) + 1, nullptr);
    }
    if(table[static_cast<size_t>(device)] == nullptr) {
        table[static_cast<size_t>(device)] = new LightProbeWorkspace();
    }
    return *table[static_cast<size_t>(device)];
}

// ws.mutex held: what the latest device-form call left running has ended
int settle(LightProbeWorkspace &ws) {
    if(ws.pending) {
        PT_HIP(hipEventSynchronize(ws.last));
        ws.pending = false;
    }
    return PT_OK;
}

int check_params(const pt_light_probe_params *p, uint64_t n) {
    if(p->samples < 1) {
        return fail(PT_ERR_INVALID, "samples must be at least 1");
    }
    if(n > LIGHT_PROBE_MAX || n * static_cast<uint64_t>(p->samples) > LIGHT_PROBE_MAX) {
        return fail(PT_ERR_INVALID, "too many samples in one call: probes x samples above 0x7fffffff");
    }
    if(!(p->epsilon >= 0.0F)) {
        return fail(PT_ERR_INVALID, "epsilon must not be negative");
    }
    if(!(p->max_backfacing >= 0.0F)) {
        return fail(PT_ERR_INVALID, "max_backfacing must not be negative");
    }
    return PT_OK;
}

// *n_out = the grid's probes
int check_grid(const pt_light_probe_grid *g, uint64_t *n_out) {
    uint64_t n = 1;
    for(int a = 0; a < 3; a++) {
        if(g->count[a] == 0) {
            return fail(PT_ERR_INVALID, "a grid count must not be zero");
        }
        if(!std::isfinite(g->step[a]) || g->step[a] == 0.0F) {
            return fail(PT_ERR_INVALID, "a grid step must be finite and not zero");
        }
        n *= g->count[a];
        if(n > LIGHT_PROBE_MAX) {
            return fail(PT_ERR_INVALID, "too many probes in a grid: above 0x7fffffff");
        }
    }
    *n_out = n;
    return PT_OK;
}

int check_points(pt_scene *s, const float *positions, size_t n, const pt_light_probe_params *params, const pt_light_probe *out) {
    if(s == nullptr || params == nullptr || (n > 0 && (positions == nullptr || out == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    return check_params(params, n);
}

int check_shade(pt_scene *s, const pt_light_probe_grid *grid, const pt_light_probe *probes, const pt_light_probe_params *params, const float *points, size_t n, const float *out,
                uint64_t *n_probes) {
    if(s == nullptr || grid == nullptr || probes == nullptr || params == nullptr || (n > 0 && (points == nullptr || out == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    PT_TRY(check_grid(grid, n_probes));
    if(n > LIGHT_PROBE_MAX) {
        return fail(PT_ERR_INVALID, "too many points in one call: above 0x7fffffff");
    }
    if(!(params->max_backfacing >= 0.0F)) {
        return fail(PT_ERR_INVALID, "max_backfacing must not be negative");
    }
    return PT_OK;
}

PtLightProbeGrid device_grid(const pt_light_probe_grid *g) {
    PtLightProbeGrid out{};
    for(int a = 0; a < 3; a++) {
        out.origin[a] = g != nullptr ? g->origin[a] : 0.0F;
        out.step[a] = g != nullptr ? g->step[a] : 1.0F;
        out.count[a] = g != nullptr ? g->count[a] : 1U;
    }
    return out;
}

// Probes per launch: whole probes, PT_LIGHT_PROBE_CHUNK pairs at the most, one probe where a probe alone has more
size_t chunk_probes(const pt_light_probe_params *p) {
    const int pairs = std::max(env_int("PT_LIGHT_PROBE_CHUNK", LIGHT_PROBE_CHUNK_DEFAULT), 1);
    return std::max<size_t>(static_cast<size_t>(pairs) / static_cast<size_t>(p->samples), 1);
}

// The launch configuration and the workspace of a call of n probes (render_mutex held, the device set)
int prepare(pt_scene *s, LightProbeWorkspace &ws, size_t n, const pt_light_probe_params *p, PtPathConfig *cfg) {
    PT_TRY(settle(ws));
    PT_TRY(setup_path(s));
    *cfg = s->path_cfg;
    const size_t pairs = std::min(n, chunk_probes(p)) * static_cast<size_t>(p->samples);
    PT_HIP(ws.spill.ensure(((pairs + 255) / 256) * 256 * cfg->spill_depth));
    cfg->spill = ws.spill.ptr;
    PT_HIP(ws.plane.ensure(2 * pairs));
    return PT_OK;
}

// Enqueues the launches of n probes on the scene's stream; d_positions == null: the grid's nodes
void enqueue(pt_scene *s, LightProbeWorkspace &ws, const PtPathConfig &cfg, const pt_light_probe_params *p, const float *d_positions, const PtLightProbeGrid &grid, size_t n,
             pt_light_probe *d_out) {
    const size_t step = chunk_probes(p);
    for(size_t first = 0; first < n; first += step) {
        pt_launch_light_probes(s->stream, s->dev, d_positions, grid, static_cast<uint32_t>(first), static_cast<uint32_t>(std::min(step, n - first)),
                               static_cast<uint32_t>(p->samples), p->epsilon, p->base_seed, reinterpret_cast<float4 *>(ws.plane.ptr), reinterpret_cast<float4 *>(d_out), cfg);
    }
}

// Host form: what `enqueue_all` puts on the scene's stream, then `bytes` from `from` into `out`.  Device form: the same between the two
// halves of a StreamOrder (pt_gather.cpp's arrangement).
template<typename Enqueue>
int run_host(pt_scene *s, void *out, const void *from, size_t bytes, Enqueue enqueue_all) {
    StreamDrain drain{s->stream};
    enqueue_all();
    PT_HIP(hipGetLastError());
    PT_HIP(hipMemcpyAsync(out, from, bytes, hipMemcpyDeviceToHost, s->stream));
    drain.armed = false;
    PT_HIP(hipStreamSynchronize(s->stream));
    return PT_OK;
}

template<typename Enqueue>
int run_device(pt_scene *s, LightProbeWorkspace &ws, void *stream, Enqueue enqueue_all) {
    StreamOrder order;
    PT_TRY(order.begin(stream, s->stream));
    enqueue_all();
    PT_HIP(hipGetLastError());
    if(ws.last == nullptr) {
        PT_HIP(hipEventCreateWithFlags(&ws.last, hipEventDisableTiming));
    }
    PT_HIP(hipEventRecord(ws.last, s->stream));
    ws.pending = true;
    PT_TRY(order.end());
    if(order.caller == nullptr) {
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    return PT_OK;
}

} // namespace

extern "C" {

int pt_light_probe_params_default(pt_light_probe_params *out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    out->samples = 256;
    out->epsilon = 1.0e-3F;
    out->base_seed = 0;
    out->max_backfacing = 0.25F;
    out->pad = 0;
    return PT_OK;
}

int pt_light_probes_points(pt_scene *s, const float *positions, size_t n, const pt_light_probe_params *params, pt_light_probe *out) {
    PT_TRY(check_points(s, positions, n, params, out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    LightProbeWorkspace &ws = workspace(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    PtPathConfig cfg;
    PT_TRY(prepare(s, ws, n, params, &cfg));
    PT_HIP(ws.positions.ensure(3 * n));
    PT_HIP(ws.out.ensure(n));
    PT_HIP(hipMemcpyAsync(ws.positions.ptr, positions, 3 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    return run_host(s, out, ws.out.ptr, n * sizeof(pt_light_probe), [&] { enqueue(s, ws, cfg, params, ws.positions.ptr, device_grid(nullptr), n, ws.out.ptr); });
}

int pt_light_probes_points_device(pt_scene *s, const float *d_positions, size_t n, const pt_light_probe_params *params, pt_light_probe *d_out, void *stream) {
    PT_TRY(check_points(s, d_positions, n, params, d_out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    LightProbeWorkspace &ws = workspace(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    PtPathConfig cfg;
    PT_TRY(prepare(s, ws, n, params, &cfg));
    return run_device(s, ws, stream, [&] { enqueue(s, ws, cfg, params, d_positions, device_grid(nullptr), n, d_out); });
}

int pt_light_probes_grid(pt_scene *s, const pt_light_probe_grid *grid, const pt_light_probe_params *params, pt_light_probe *out) {
    if(s == nullptr || grid == nullptr || params == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    uint64_t n64 = 0;
    PT_TRY(check_grid(grid, &n64));
    PT_TRY(check_params(params, n64));
    const size_t n = static_cast<size_t>(n64);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    LightProbeWorkspace &ws = workspace(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    PtPathConfig cfg;
    PT_TRY(prepare(s, ws, n, params, &cfg));
    PT_HIP(ws.out.ensure(n));
    return run_host(s, out, ws.out.ptr, n * sizeof(pt_light_probe), [&] { enqueue(s, ws, cfg, params, nullptr, device_grid(grid), n, ws.out.ptr); });
}

int pt_light_probes_shade(pt_scene *s, const pt_light_probe_grid *grid, const pt_light_probe *probes, const pt_light_probe_params *params, const float *points, size_t n,
                          float *out) {
    uint64_t n_probes = 0;
    PT_TRY(check_shade(s, grid, probes, params, points, n, out, &n_probes));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    LightProbeWorkspace &ws = workspace(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    PT_TRY(settle(ws));
    PT_HIP(ws.out.ensure(n_probes));
    PT_HIP(ws.points.ensure(6 * n));
    PT_HIP(ws.values.ensure(n));
    PT_HIP(hipMemcpyAsync(ws.out.ptr, probes, n_probes * sizeof(pt_light_probe), hipMemcpyHostToDevice, s->stream));
    PT_HIP(hipMemcpyAsync(ws.points.ptr, points, 6 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    return run_host(s, out, ws.values.ptr, n * sizeof(F4), [&] {
        pt_launch_light_probe_shade(s->stream, device_grid(grid), reinterpret_cast<const float4 *>(ws.out.ptr), params->max_backfacing, ws.points.ptr, static_cast<uint32_t>(n),
                                    reinterpret_cast<float4 *>(ws.values.ptr));
    });
}

int pt_light_probes_shade_device(pt_scene *s, const pt_light_probe_grid *grid, const pt_light_probe *d_probes, const pt_light_probe_params *params, const float *d_points, size_t n,
                                 float *d_out, void *stream) {
    uint64_t n_probes = 0;
    PT_TRY(check_shade(s, grid, d_probes, params, d_points, n, d_out, &n_probes));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    StreamOrder order; // (the lookup's device form uses no buffer of the workspace)
    PT_TRY(order.begin(stream, s->stream));
    pt_launch_light_probe_shade(s->stream, device_grid(grid), reinterpret_cast<const float4 *>(d_probes), params->max_backfacing, d_points, static_cast<uint32_t>(n),
                                reinterpret_cast<float4 *>(d_out));
    PT_HIP(hipGetLastError());
    PT_TRY(order.end());
    if(order.caller == nullptr) {
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    return PT_OK;
}

} // extern "C"
