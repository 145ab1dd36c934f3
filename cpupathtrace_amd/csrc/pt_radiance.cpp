// pt_radiance.cpp -- the entry points of include/pt_radiance.h: the radiance along rays the caller chooses, and captures --
// images of such rays made on the device by one of four camera models.  The kernels are pt_radiance_kernels.h's (in pt_walks.hip); this
// unit checks the arguments, keeps the workspace -- one per device, grown on demand, as pt_light_probes.cpp keeps its own; pt_scene is as
// it was -- and cuts a call into launches of whole rays or pixels: at most PT_RADIANCE_CHUNK (ray or pixel, sample) pairs each, read per
// call.  A sample's engine is seeded with its ray's or pixel's index in the call, and a record is reduced in an order of its own, so the
// cut changes no bit.  Nothing here changes the scene, so every call is allowed with a live pt_frame and with or without a motion mark.
#include "pt_host.h"

#include <cmath>

using namespace pth;

namespace {

const uint64_t RADIANCE_MAX = 0x7fffffffULL;
const int RADIANCE_CHUNK_DEFAULT = 2 << 20;

// The buffers of the calls on one device: the host forms' rays and records, and the workspace of one launch -- one float4 per pair and
// the walks' spill area.  One call at a time per device (`mutex`, taken behind the scene's render lock); `last` marks the end of the
// latest device-form call, whose work may still run when the next call comes: that call waits for it before it touches a buffer.  Lives
// as long as the process (never freed: a static destructor would run after the HIP runtime has gone).
struct RadianceWorkspace {
    std::mutex mutex;
    DevBuf<float> rays;
    DevBuf<pt_radiance_result> out;
    DevBuf<F4> plane;
    DevBuf<uint2> spill;
    hipEvent_t last = nullptr;
    bool pending = false;
};

RadianceWorkspace &workspace(int device) {
    static std::mutex table_mutex;
    static std::vector<RadianceWorkspace *> table;
    std::lock_guard<std::mutex> lock(table_mutex);
    if(static_cast<size_t>(device) >= table.size()) {
        table.resize(static_cast<size_t>(device) + 1, nullptr);
    }
    if(table[static_cast<size_t>(device)] == nullptr) {
        table[static_cast<size_t>(device)] = new RadianceWorkspace();
    }
    return *table[static_cast<size_t>(device)];
}

// ws.mutex held: what the latest device-form call left running has ended
int settle(RadianceWorkspace &ws) {
    if(ws.pending) {
        PT_HIP(hipEventSynchronize(ws.last));
        ws.pending = false;
    }
    return PT_OK;
}

} // namespace

// The argument checks and the capture as the kernels take it, shared with pt_light_passes.cpp (declared in pt_host.h)
namespace pth {

int radiance_check_params(const pt_radiance_params *p, uint64_t n) {
    if(p->samples < 1) {
        return fail(PT_ERR_INVALID, "samples must be at least 1");
    }
    if(n > RADIANCE_MAX || n * static_cast<uint64_t>(p->samples) > RADIANCE_MAX) {
        return fail(PT_ERR_INVALID, "too many samples in one call: rays or pixels x samples above 0x7fffffff");
    }
    if(!(p->epsilon >= 0.0F)) {
        return fail(PT_ERR_INVALID, "epsilon must not be negative");
    }
    return PT_OK;
}

int radiance_check_rays(pt_scene *s, const float *rays, size_t n, const pt_radiance_params *params, const void *out) {
    if(s == nullptr || params == nullptr || (n > 0 && (rays == nullptr || out == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    return radiance_check_params(params, n);
}

// *n_out = the capture's pixels
int radiance_check_capture(pt_scene *s, const pt_capture_desc *c, const pt_radiance_params *params, const void *out, uint64_t *n_out) {
    if(s == nullptr || c == nullptr || params == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(c->model != PT_CAPTURE_EQUIRECT && c->model != PT_CAPTURE_CUBE && c->model != PT_CAPTURE_FISHEYE && c->model != PT_CAPTURE_ORTHO) {
        return fail(PT_ERR_INVALID, "unknown capture model");
    }
    if(c->width < 1 || c->height < 1) {
        return fail(PT_ERR_INVALID, "a capture's width and height must be at least 1");
    }
    if(c->jitter != 0 && c->jitter != 1) {
        return fail(PT_ERR_INVALID, "jitter must be 0 or 1");
    }
    if(c->model == PT_CAPTURE_CUBE && static_cast<int64_t>(c->width) != 6 * static_cast<int64_t>(c->height)) {
        return fail(PT_ERR_INVALID, "a cube capture is six square faces side by side: width must be 6 * height");
    }
    if(c->model == PT_CAPTURE_FISHEYE) {
        if(c->width != c->height) {
            return fail(PT_ERR_INVALID, "a fisheye capture is square: width must equal height");
        }
        // (2 pi as fp32 has it, 2.0f * PT_PI_F: the largest angle a caller can mean by it)
        if(!(c->fov > 0.0F) || !(c->fov <= 2.0F * 3.14159274101257324219F)) {
            return fail(PT_ERR_INVALID, "a fisheye's fov must be above 0 and at most 2 pi");
        }
    }
    if(c->model == PT_CAPTURE_ORTHO) {
        for(int a = 0; a < 2; a++) {
            if(!std::isfinite(c->extent[a]) || !(c->extent[a] > 0.0F)) {
                return fail(PT_ERR_INVALID, "an orthographic extent must be finite and above 0");
            }
        }
    }
    for(int k = 0; k < 3; k++) {
        if(!std::isfinite(c->origin[k]) || !std::isfinite(c->right[k]) || !std::isfinite(c->up[k]) || !std::isfinite(c->forward[k])) {
            return fail(PT_ERR_INVALID, "a capture's origin and basis must be finite");
        }
    }
    *n_out = static_cast<uint64_t>(c->width) * static_cast<uint64_t>(c->height);
    return radiance_check_params(params, *n_out);
}

PtCaptureParams radiance_device_capture(const pt_capture_desc *c) {
    PtCaptureParams out{};
    if(c == nullptr) {
        out.width = out.height = 1;
        return out;
    }
    out.model = c->model;
    out.width = c->width;
    out.height = c->height;
    out.jitter = c->jitter;
    for(int k = 0; k < 3; k++) {
        out.origin[k] = c->origin[k];
        out.right[k] = c->right[k];
        out.up[k] = c->up[k];
        out.forward[k] = c->forward[k];
    }
    out.fov = c->fov;
    out.extent[0] = c->extent[0];
    out.extent[1] = c->extent[1];
    return out;
}

} // namespace pth

namespace {

// Rays or pixels per launch: whole ones, PT_RADIANCE_CHUNK pairs at the most, one where one alone has more
size_t chunk_items(const pt_radiance_params *p) {
    const int pairs = std::max(env_int("PT_RADIANCE_CHUNK", RADIANCE_CHUNK_DEFAULT), 1);
    return std::max<size_t>(static_cast<size_t>(pairs) / static_cast<size_t>(p->samples), 1);
}

// The launch configuration and the workspace of a call of n rays or pixels cut by `step` (render_mutex held, the device set)
int prepare(pt_scene *s, RadianceWorkspace &ws, size_t n, size_t step, const pt_radiance_params *p, PtPathConfig *cfg) {
    PT_TRY(settle(ws));
    PT_TRY(setup_path(s));
    *cfg = s->path_cfg;
    const size_t pairs = std::min(n, step) * static_cast<size_t>(p->samples);
    PT_HIP(ws.spill.ensure(((pairs + 255) / 256) * 256 * cfg->spill_depth));
    cfg->spill = ws.spill.ptr;
    PT_HIP(ws.plane.ensure(pairs));
    return PT_OK;
}

// Enqueues the launches of n rays or pixels on the scene's stream; d_rays == null: the capture's pixels
void enqueue(pt_scene *s, RadianceWorkspace &ws, const PtPathConfig &cfg, const pt_radiance_params *p, size_t step, const float *d_rays, const PtCaptureParams &capture, size_t n,
             pt_radiance_result *d_out) {
    for(size_t first = 0; first < n; first += step) {
        pt_launch_radiance(s->stream, s->dev, d_rays, capture, static_cast<uint32_t>(first), static_cast<uint32_t>(std::min(step, n - first)), static_cast<uint32_t>(p->samples),
                           p->epsilon, p->base_seed, reinterpret_cast<float4 *>(ws.plane.ptr), reinterpret_cast<float4 *>(d_out), cfg);
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
int run_device(pt_scene *s, RadianceWorkspace &ws, void *stream, Enqueue enqueue_all) {
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

// A call of n rays (d_rays or, host form, rays) or of the capture's n pixels (both null); host form: d_out == null, the records go to `out`
int run(pt_scene *s, const float *rays, const float *d_rays, const pt_capture_desc *capture, size_t n, const pt_radiance_params *params, pt_radiance_result *out,
        pt_radiance_result *d_out, void *stream) {
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    RadianceWorkspace &ws = workspace(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    const size_t step = chunk_items(params);
    PtPathConfig cfg;
    PT_TRY(prepare(s, ws, n, step, params, &cfg));
    const PtCaptureParams cap = radiance_device_capture(capture);
    if(d_out != nullptr) {
        return run_device(s, ws, stream, [&] { enqueue(s, ws, cfg, params, step, d_rays, cap, n, d_out); });
    }
    PT_HIP(ws.out.ensure(n));
    if(rays != nullptr) {
        PT_HIP(ws.rays.ensure(6 * n));
        PT_HIP(hipMemcpyAsync(ws.rays.ptr, rays, 6 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    }
    return run_host(s, out, ws.out.ptr, n * sizeof(pt_radiance_result), [&] { enqueue(s, ws, cfg, params, step, rays != nullptr ? ws.rays.ptr : nullptr, cap, n, ws.out.ptr); });
}

} // namespace

extern "C" {

int pt_radiance_params_default(pt_radiance_params *out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    out->samples = 64;
    out->epsilon = 1.0e-3F;
    out->base_seed = 0;
    return PT_OK;
}

int pt_radiance_rays(pt_scene *s, const float *rays, size_t n, const pt_radiance_params *params, pt_radiance_result *out) {
    PT_TRY(radiance_check_rays(s, rays, n, params, out));
    if(n == 0) {
        return PT_OK;
    }
    return run(s, rays, nullptr, nullptr, n, params, out, nullptr, nullptr);
}

int pt_radiance_rays_device(pt_scene *s, const float *d_rays, size_t n, const pt_radiance_params *params, pt_radiance_result *d_out, void *stream) {
    PT_TRY(radiance_check_rays(s, d_rays, n, params, d_out));
    if(n == 0) {
        return PT_OK;
    }
    return run(s, nullptr, d_rays, nullptr, n, params, nullptr, d_out, stream);
}

int pt_radiance_capture(pt_scene *s, const pt_capture_desc *capture, const pt_radiance_params *params, pt_radiance_result *out) {
    uint64_t n = 0;
    PT_TRY(radiance_check_capture(s, capture, params, out, &n));
    return run(s, nullptr, nullptr, capture, static_cast<size_t>(n), params, out, nullptr, nullptr);
}

int pt_radiance_capture_device(pt_scene *s, const pt_capture_desc *capture, const pt_radiance_params *params, pt_radiance_result *d_out, void *stream) {
    uint64_t n = 0;
    PT_TRY(radiance_check_capture(s, capture, params, d_out, &n));
    return run(s, nullptr, nullptr, capture, static_cast<size_t>(n), params, nullptr, d_out, stream);
}

} // extern "C"
