// pt_gather.cpp -- the entry points of include/pt_gather.h: light gathered at points, at a frame's first hits and at the
// corners of an instance's triangles.  The kernels are pt_gather_kernels.h's (in pt_walks.hip); this unit checks the arguments, keeps the
// workspace on the scene (grown on demand, freed with it) and cuts a call into launches of whole points: at most PT_GATHER_CHUNK (point,
// sample) pairs each, read per call.  A sample's engine is seeded with its point's index in the call, so the cut changes no bit.
// Nothing here changes the scene, so every call is allowed with a live pt_frame and with or without a motion mark.
#include "pt_sample_host.h"

#include <limits>

using namespace pth;

namespace {

const uint64_t GATHER_MAX = 0x7fffffffULL;

int check_params(const pt_gather_params *p, uint64_t n) {
    if(p->kind != PT_GATHER_OCCLUSION && p->kind != PT_GATHER_DIRECT && p->kind != PT_GATHER_PATHS) {
        return fail(PT_ERR_INVALID, "unknown gather kind " + std::to_string(p->kind));
    }
    if(p->samples < 1) {
        return fail(PT_ERR_INVALID, "samples must be at least 1");
    }
    if(n * static_cast<uint64_t>(p->samples) > GATHER_MAX) {
        return fail(PT_ERR_INVALID, "too many samples in one call: points x samples above 0x7fffffff");
    }
    if(!(p->epsilon >= 0.0F)) {
        return fail(PT_ERR_INVALID, "epsilon must not be negative");
    }
    if(p->kind == PT_GATHER_OCCLUSION && !(p->distance > 0.0F)) {
        return fail(PT_ERR_INVALID, "the occlusion distance must be greater than 0");
    }
    return PT_OK;
}

int check_points(pt_scene *s, const float *points, size_t n, const pt_gather_params *params, const pt_gather_result *out) {
    if(s == nullptr || params == nullptr || (n > 0 && (points == nullptr || out == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(n > GATHER_MAX) {
        return fail(PT_ERR_INVALID, "too many samples in one call: points x samples above 0x7fffffff");
    }
    return check_params(params, n);
}

int check_frame(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_gather_params *params, const pt_gather_result *out) {
    PT_TRY(check_render_args(s, camera, options));
    if(params == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    return check_params(params, static_cast<uint64_t>(options->image_width) * static_cast<uint64_t>(options->image_height));
}

// Points per launch (PT_GATHER_CHUNK)
size_t chunk_points(const pt_gather_params *p) {
    return chunk_items("PT_GATHER_CHUNK", GATHER_CHUNK_DEFAULT, p->samples, 1);
}

// The launch configuration and the workspace of a call of n points (render_mutex held, the device set); `walks`: walks of a launch
// that makes the points, which shares the spill area.  The buffers live on the scene and are ordered by its stream.
int prepare(pt_scene *s, size_t n, const pt_gather_params *p, size_t walks, PtPathConfig *cfg) {
    const size_t pairs = std::min(n, chunk_points(p)) * static_cast<size_t>(p->samples);
    const bool bits = p->kind == PT_GATHER_OCCLUSION;
    PT_TRY(size_launch(s, s->gather_spill, std::max(pairs, walks), bits ? nullptr : &s->gather_plane, pairs, cfg));
    if(bits) {
        PT_HIP(s->gather_bits.ensure((pairs + 63) / 64));
    }
    return PT_OK;
}

// Enqueues the launches of n points on the scene's stream and, host form (out != null), the n records' way to `out`
int enqueue(pt_scene *s, const PtPathConfig &cfg, const pt_gather_params *p, const float *d_points, const uint8_t *d_miss, size_t n, pt_gather_result *d_out,
            pt_gather_result *out = nullptr) {
    const size_t step = chunk_points(p);
    for(size_t first = 0; first < n; first += step) {
        pt_launch_gather(s->stream, s->dev, p->kind, d_points, d_miss, static_cast<uint32_t>(first), static_cast<uint32_t>(std::min(step, n - first)),
                         static_cast<uint32_t>(p->samples), p->epsilon, p->distance, p->base_seed, reinterpret_cast<float4 *>(s->gather_plane.ptr), s->gather_bits.ptr,
                         reinterpret_cast<float4 *>(d_out), cfg);
    }
    if(out != nullptr) {
        PT_HIP(hipMemcpyAsync(out, d_out, n * sizeof(pt_gather_result), hipMemcpyDeviceToHost, s->stream));
    }
    return PT_OK;
}

PtDevCamera pixel_camera(const pt_camera_params *camera) {
    PtDevCamera cam = derive_camera(camera);
    cam.aperture_kind = PT_APERTURE_NONE; // the rays are a pure function of camera and pixel
    return cam;
}

} // namespace

extern "C" {

int pt_gather_params_default(pt_gather_params *out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    out->kind = PT_GATHER_OCCLUSION;
    out->samples = 16;
    out->epsilon = 1.0e-3F;
    out->distance = std::numeric_limits<float>::infinity();
    out->base_seed = 0;
    return PT_OK;
}

int pt_gather_points(pt_scene *s, const float *points, size_t n, const pt_gather_params *params, pt_gather_result *out) {
    PT_TRY(check_points(s, points, n, params, out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PT_TRY(prepare(s, n, params, 0, &cfg));
    PT_HIP(s->gather_points.ensure(6 * n));
    PT_HIP(s->gather_out.ensure(n));
    return run_host(s, [&]() -> int {
        PT_HIP(hipMemcpyAsync(s->gather_points.ptr, points, 6 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
        return enqueue(s, cfg, params, s->gather_points.ptr, nullptr, n, s->gather_out.ptr, out);
    });
}

int pt_gather_points_device(pt_scene *s, const float *d_points, size_t n, const pt_gather_params *params, pt_gather_result *d_out, void *stream) {
    PT_TRY(check_points(s, d_points, n, params, d_out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PT_TRY(prepare(s, n, params, 0, &cfg));
    return run_device(s, nullptr, stream, [&]() -> int { return enqueue(s, cfg, params, d_points, nullptr, n, d_out); });
}

int pt_gather_frame(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_gather_params *params, pt_gather_result *out) {
    PT_TRY(check_frame(s, camera, options, params, out));
    const size_t n = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PT_TRY(prepare(s, n, params, n, &cfg));
    PT_HIP(s->gather_points.ensure(6 * n));
    PT_HIP(s->gather_miss.ensure(n));
    PT_HIP(s->gather_out.ensure(n));
    const PtDevCamera cam = pixel_camera(camera);
    return run_host(s, [&]() -> int {
        pt_launch_gather_frame_points(s->stream, s->dev, cam, options->image_width, options->image_height, s->gather_points.ptr, s->gather_miss.ptr, cfg);
        return enqueue(s, cfg, params, s->gather_points.ptr, s->gather_miss.ptr, n, s->gather_out.ptr, out);
    });
}

int pt_gather_frame_device(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_gather_params *params, pt_gather_result *d_out, void *stream) {
    PT_TRY(check_frame(s, camera, options, params, d_out));
    const size_t n = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PT_TRY(prepare(s, n, params, n, &cfg));
    PT_HIP(s->gather_points.ensure(6 * n));
    PT_HIP(s->gather_miss.ensure(n));
    const PtDevCamera cam = pixel_camera(camera);
    return run_device(s, nullptr, stream, [&]() -> int {
        pt_launch_gather_frame_points(s->stream, s->dev, cam, options->image_width, options->image_height, s->gather_points.ptr, s->gather_miss.ptr, cfg);
        return enqueue(s, cfg, params, s->gather_points.ptr, s->gather_miss.ptr, n, d_out);
    });
}

int pt_gather_instance(pt_scene *s, uint32_t instance, const pt_gather_params *params, pt_gather_result *out) {
    if(s == nullptr || params == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(instance >= s->inst_first.size()) {
        return fail(PT_ERR_INVALID, "instance " + std::to_string(instance) + " out of range: the scene has " + std::to_string(s->inst_first.size()));
    }
    const uint32_t n_tris = s->inst_count[instance];
    const size_t n = 3 * static_cast<size_t>(n_tris);
    PT_TRY(check_params(params, n));
    if(n == 0) {
        return PT_OK;
    }
    if(s->tri_pos_kept.ptr == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, "the scene keeps no triangle arrays: it was not made by pt_scene_create_meshes with instances");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PT_TRY(prepare(s, n, params, 0, &cfg));
    PT_HIP(s->gather_points.ensure(6 * n));
    PT_HIP(s->gather_out.ensure(n));
    const uint32_t first_tri = s->n_desc_tris + (s->inst_first[instance] - s->n_desc_objects); // (pt_scene_get_triangles' triangle of an instance's object)
    return run_host(s, [&]() -> int {
        pt_launch_gather_corner_points(s->stream, s->tri_pos_kept.ptr, reinterpret_cast<const float4 *>(s->tri_shade.ptr), first_tri, n_tris, s->gather_points.ptr);
        return enqueue(s, cfg, params, s->gather_points.ptr, nullptr, n, s->gather_out.ptr, out);
    });
}

} // extern "C"
