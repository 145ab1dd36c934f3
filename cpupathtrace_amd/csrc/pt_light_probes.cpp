// pt_light_probes.cpp -- the entry points of include/pt_light_probes.h: SH radiance at free points, at the nodes of a grid,
// and the lookup that shades points from a grid's records.  The kernels are pt_light_probe_kernels.h's (in pt_walks.hip); this unit checks
// the arguments, keeps the workspace -- one per device, grown on demand, as the denoiser keeps its own (pt_image.cpp); pt_scene is as it
// was -- and cuts a call into launches of whole probes: at most PT_LIGHT_PROBE_CHUNK (probe, sample) pairs each, read per call.  A
// sample's engine is seeded with its probe's index in the call, and a probe's record is reduced in an order of its own, so the cut
// changes no bit.  The launch frame -- workspace table, chunk rule, sizing, the two brackets -- is pt_sample_host.h's.  Nothing here
// changes the scene, so every call is allowed with a live pt_frame and with or without a motion mark.
#include "pt_sample_host.h"

#include <cmath>

using namespace pth;

namespace {

const uint64_t LIGHT_PROBE_MAX = 0x7fffffffULL;

// The buffers of the calls on one device beside the workspace of one launch (two float4 per (probe, sample) pair in the plane): the
// host forms' positions, records, points and values
struct LightProbeWorkspace : SampleWorkspace {
    DevBuf<float> positions;
    DevBuf<pt_light_probe> out;
    DevBuf<float> points;
    DevBuf<F4> values;
};

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

// Probes per launch (PT_LIGHT_PROBE_CHUNK)
size_t chunk_probes(const pt_light_probe_params *p) {
    return chunk_items("PT_LIGHT_PROBE_CHUNK", LIGHT_PROBE_CHUNK_DEFAULT, p->samples, 1);
}

// The launch configuration and the workspace of a call of n probes (render_mutex and ws.mutex held, the device set)
int prepare(pt_scene *s, LightProbeWorkspace &ws, size_t n, const pt_light_probe_params *p, PtPathConfig *cfg) {
    PT_TRY(settle(ws));
    const size_t pairs = std::min(n, chunk_probes(p)) * static_cast<size_t>(p->samples);
    return size_launch(s, ws.spill, pairs, &ws.plane, 2 * pairs, cfg);
}

// Enqueues the launches of n probes on the scene's stream; d_positions == null: the grid's nodes.  Host form (out != null): then the
// n records' way to `out`.
int enqueue(pt_scene *s, LightProbeWorkspace &ws, const PtPathConfig &cfg, const pt_light_probe_params *p, const float *d_positions, const PtLightProbeGrid &grid, size_t n,
            pt_light_probe *d_out, pt_light_probe *out = nullptr) {
    const size_t step = chunk_probes(p);
    for(size_t first = 0; first < n; first += step) {
        pt_launch_light_probes(s->stream, s->dev, d_positions, grid, static_cast<uint32_t>(first), static_cast<uint32_t>(std::min(step, n - first)),
                               static_cast<uint32_t>(p->samples), p->epsilon, p->base_seed, reinterpret_cast<float4 *>(ws.plane.ptr), reinterpret_cast<float4 *>(d_out), cfg);
    }
    if(out != nullptr) {
        PT_HIP(hipMemcpyAsync(out, d_out, n * sizeof(pt_light_probe), hipMemcpyDeviceToHost, s->stream));
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
    LightProbeWorkspace &ws = sample_workspace<LightProbeWorkspace>(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    PtPathConfig cfg;
    PT_TRY(prepare(s, ws, n, params, &cfg));
    PT_HIP(ws.positions.ensure(3 * n));
    PT_HIP(ws.out.ensure(n));
    return run_host(s, [&]() -> int {
        PT_HIP(hipMemcpyAsync(ws.positions.ptr, positions, 3 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
        return enqueue(s, ws, cfg, params, ws.positions.ptr, device_grid(nullptr), n, ws.out.ptr, out);
    });
}

int pt_light_probes_points_device(pt_scene *s, const float *d_positions, size_t n, const pt_light_probe_params *params, pt_light_probe *d_out, void *stream) {
    PT_TRY(check_points(s, d_positions, n, params, d_out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    LightProbeWorkspace &ws = sample_workspace<LightProbeWorkspace>(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    PtPathConfig cfg;
    PT_TRY(prepare(s, ws, n, params, &cfg));
    return run_device(s, &ws, stream, [&]() -> int { return enqueue(s, ws, cfg, params, d_positions, device_grid(nullptr), n, d_out); });
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
    LightProbeWorkspace &ws = sample_workspace<LightProbeWorkspace>(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    PtPathConfig cfg;
    PT_TRY(prepare(s, ws, n, params, &cfg));
    PT_HIP(ws.out.ensure(n));
    return run_host(s, [&]() -> int { return enqueue(s, ws, cfg, params, nullptr, device_grid(grid), n, ws.out.ptr, out); });
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
    LightProbeWorkspace &ws = sample_workspace<LightProbeWorkspace>(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    PT_TRY(settle(ws));
    PT_HIP(ws.out.ensure(n_probes));
    PT_HIP(ws.points.ensure(6 * n));
    PT_HIP(ws.values.ensure(n));
    return run_host(s, [&]() -> int {
        PT_HIP(hipMemcpyAsync(ws.out.ptr, probes, n_probes * sizeof(pt_light_probe), hipMemcpyHostToDevice, s->stream));
        PT_HIP(hipMemcpyAsync(ws.points.ptr, points, 6 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
        pt_launch_light_probe_shade(s->stream, device_grid(grid), reinterpret_cast<const float4 *>(ws.out.ptr), params->max_backfacing, ws.points.ptr, static_cast<uint32_t>(n),
                                    reinterpret_cast<float4 *>(ws.values.ptr));
        PT_HIP(hipMemcpyAsync(out, ws.values.ptr, n * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
        return PT_OK;
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
