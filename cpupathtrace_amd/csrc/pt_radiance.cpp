// pt_radiance.cpp -- the entry points of include/pt_radiance.h: the radiance along rays the caller chooses, and captures --
// images of such rays made on the device by one of four camera models.  The kernels are pt_radiance_kernels.h's (in pt_walks.hip); this
// unit checks the arguments, keeps the workspace -- one per device, grown on demand, from pt_sample_host.h's table and launch frame;
// pt_scene is as it was -- and cuts a call into launches of whole rays or pixels: at most PT_RADIANCE_CHUNK (ray or pixel, sample) pairs each, read per
// call.  A sample's engine is seeded with its ray's or pixel's index in the call, and a record is reduced in an order of its own, so the
// cut changes no bit.  Nothing here changes the scene, so every call is allowed with a live pt_frame and with or without a motion mark.
#include "pt_sample_host.h"

#include <cmath>

using namespace pth;

namespace {

const uint64_t RADIANCE_MAX = 0x7fffffffULL;

// The buffers of the calls on one device beside the workspace of one launch (one float4 per pair in the plane): the host forms' rays
// and records
struct RadianceWorkspace : SampleWorkspace {
    DevBuf<float> rays;
    DevBuf<pt_radiance_result> out;
};

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

// A call of n rays (d_rays or, host form, rays) or of the capture's n pixels (both null); host form: d_out == null, the records go to `out`
int run(pt_scene *s, const float *rays, const float *d_rays, const pt_capture_desc *capture, size_t n, const pt_radiance_params *params, pt_radiance_result *out,
        pt_radiance_result *d_out, void *stream) {
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    RadianceWorkspace &ws = sample_workspace<RadianceWorkspace>(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    const size_t step = chunk_items("PT_RADIANCE_CHUNK", RADIANCE_CHUNK_DEFAULT, params->samples, 1);
    PT_TRY(settle(ws));
    const size_t pairs = std::min(n, step) * static_cast<size_t>(params->samples);
    PtPathConfig cfg;
    PT_TRY(size_launch(s, ws.spill, pairs, &ws.plane, pairs, &cfg));
    const bool host = d_out == nullptr;
    if(host) {
        PT_HIP(ws.out.ensure(n));
        if(rays != nullptr) {
            PT_HIP(ws.rays.ensure(6 * n));
        }
    }
    const PtCaptureParams cap = radiance_device_capture(capture);
    const float *use_rays = host ? (rays != nullptr ? ws.rays.ptr : nullptr) : d_rays;
    pt_radiance_result *records = host ? ws.out.ptr : d_out;
    auto enqueue_all = [&]() -> int {
        if(host && rays != nullptr) {
            PT_HIP(hipMemcpyAsync(ws.rays.ptr, rays, 6 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
        }
        for(size_t first = 0; first < n; first += step) {
            pt_launch_radiance(s->stream, s->dev, use_rays, cap, static_cast<uint32_t>(first), static_cast<uint32_t>(std::min(step, n - first)),
                               static_cast<uint32_t>(params->samples), params->epsilon, params->base_seed, reinterpret_cast<float4 *>(ws.plane.ptr),
                               reinterpret_cast<float4 *>(records), cfg);
        }
        if(host) {
            PT_HIP(hipMemcpyAsync(out, ws.out.ptr, n * sizeof(pt_radiance_result), hipMemcpyDeviceToHost, s->stream));
        }
        return PT_OK;
    };
    if(host) {
        return run_host(s, enqueue_all);
    }
    return run_device(s, &ws, stream, enqueue_all);
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
