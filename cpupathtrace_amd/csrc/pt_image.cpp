// pt_image.cpp -- what the C ABI (include/pt_hip.h) does to a finished image: post-processing (pt_post.hip), the first-hit features of a
// frame (pt_walks.hip: pt_feature_kernel), feature-guided denoising and its temporal form (pt_denoise.hip).  A single frame is the batch
// of one view: the single-frame entry points call the view forms with n_views = 1, which issue the single frame's launches.
#include "pt_host.h"

using namespace pth;

// ---- post-processing (pt_post.hip) ----------------------------------------------------------------------------------------------

static int post_check(int device, const float *rgba, int32_t width, int32_t height, uint32_t steps, float gamma) {
    if(width < 0 || height < 0 || (rgba == nullptr && static_cast<long long>(width) * height > 0)) {
        return fail(PT_ERR_INVALID, "bad image");
    }
    if((steps & ~(PT_POST_TONE_MAP | PT_POST_GAMMA)) != 0 || steps == 0) {
        return fail(PT_ERR_INVALID, "steps must be PT_POST_TONE_MAP and/or PT_POST_GAMMA");
    }
    if((steps & PT_POST_GAMMA) != 0 && !(gamma == gamma)) {
        return fail(PT_ERR_INVALID, "gamma is NaN");
    }
    return check_device(device);
}

extern "C" {

int pt_post_process_device(int device, float *d_rgba, int32_t width, int32_t height, uint32_t steps, float gamma, void *stream) {
    PT_TRY(post_check(device, d_rgba, width, height, steps, gamma));
    PT_HIP(hipSetDevice(device));
    static_assert(PT_POST_TONE_MAP == PT_POST_STEP_TONE_MAP && PT_POST_GAMMA == PT_POST_STEP_GAMMA, "step bits");
    PT_HIP(pt_post_run(static_cast<hipStream_t>(stream), reinterpret_cast<float4 *>(d_rgba), width, height, steps, gamma));
    return PT_OK;
}

int pt_post_process(int device, float *rgba, int32_t width, int32_t height, uint32_t steps, float gamma) {
    PT_TRY(post_check(device, rgba, width, height, steps, gamma));
    const size_t count = static_cast<size_t>(width) * static_cast<size_t>(height);
    if(count == 0) {
        return PT_OK;
    }
    PT_HIP(hipSetDevice(device));
    DevBuf<F4> frame;
    PT_HIP(frame.ensure(count));
    PT_HIP(hipMemcpy(frame.ptr, rgba, count * sizeof(F4), hipMemcpyHostToDevice));
    PT_HIP(pt_post_run(nullptr, reinterpret_cast<float4 *>(frame.ptr), width, height, steps, gamma));
    PT_HIP(hipMemcpy(rgba, frame.ptr, count * sizeof(F4), hipMemcpyDeviceToHost));
    return PT_OK;
}

} // extern "C"

// ---- feature-guided denoising (pt_walks.hip: pt_feature_kernel; pt_denoise.hip) -------------------------------------------------------

// The arguments of the feature entry points, checked without a device
static int features_views_check(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, const float *out) {
    if(n_views <= 0) {
        return fail(PT_ERR_INVALID, "a view batch needs at least one view");
    }
    if(options != nullptr && options->image_width > 0 && options->image_height > 0 &&
       static_cast<uint64_t>(n_views) * static_cast<uint64_t>(options->image_height) * static_cast<uint64_t>(options->image_width) > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    PT_TRY(check_render_args(s, cameras, options));
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    return PT_OK;
}

int pth::feature_params_resolve(const pt_feature_params *params, const pt_options *options, pt_feature_params *resolved) {
    pt_feature_params p{};
    pt_feature_params_default(&p);
    if(params != nullptr) {
        p = *params;
    }
    if(p.max_bounces < 0 || p.max_bounces > 32) {
        return fail(PT_ERR_INVALID, "max_bounces must be 0..32");
    }
    if(p.flags != 0) {
        return fail(PT_ERR_INVALID, "flags must be 0");
    }
    if(options != nullptr && !(std::isfinite(options->epsilon) && options->epsilon >= 0.0F)) {
        return fail(PT_ERR_INVALID, "epsilon must be finite and not negative");
    }
    *resolved = p;
    return PT_OK;
}

// Enqueues the feature pass on the scene's stream (render_mutex held): into `d_out`, n_views * width * height * 3 float4.  A single frame's
// camera travels in the kernel's arguments; a batch's cameras go through a device table, which costs an upload and a wait for it.
int pth::features_views_launch(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, float4 *d_out,
                               const pt_feature_params *follow) {
    PT_TRY(setup_path(s));
    std::vector<PtViewCamera> table(static_cast<size_t>(n_views));
    for(int32_t v = 0; v < n_views; v++) {
        table[static_cast<size_t>(v)] = PtViewCamera{derive_camera(cameras + v), {0, 0, 0}};
        table[static_cast<size_t>(v)].cam.aperture_kind = PT_APERTURE_NONE; // the rays are a pure function of camera and pixel
    }
    const PtViewCamera *d_views = nullptr;
    if(n_views > 1) {
        PT_HIP(s->feature_cams.ensure(table.size()));
        PT_HIP(hipMemcpyAsync(s->feature_cams.ptr, table.data(), table.size() * sizeof(PtViewCamera), hipMemcpyHostToDevice, s->stream));
        PT_HIP(hipStreamSynchronize(s->stream)); // the table is this function's vector
        d_views = s->feature_cams.ptr;
    }
    PtPathConfig cfg = s->path_cfg;
    const size_t n = static_cast<size_t>(n_views) * static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    PT_HIP(s->feature_spill.ensure(((n + 255) / 256) * 256 * cfg.spill_depth));
    cfg.spill = s->feature_spill.ptr;
    const PtFollow followed = {follow != nullptr ? follow->max_bounces : 0, options->epsilon};
    pt_launch_features(s->stream, s->dev, table[0].cam, d_views, n_views, options->image_width, options->image_height, d_out, cfg, follow != nullptr ? &followed : nullptr);
    PT_HIP(hipGetLastError());
    return PT_OK;
}

namespace pth {

DenoiseWorkspace &denoise_workspace(int device) {
    static std::mutex table_mutex;
    static std::vector<DenoiseWorkspace *> table;
    std::lock_guard<std::mutex> lock(table_mutex);
    if(static_cast<size_t>(device) >= table.size()) {
        table.resize(static_cast<size_t>(device) + 1, nullptr);
    }
    if(table[static_cast<size_t>(device)] == nullptr) {
        table[static_cast<size_t>(device)] = new DenoiseWorkspace();
    }
    return *table[static_cast<size_t>(device)];
}

template<typename T>
hipError_t regrow(T **p, size_t count) {
    if(*p != nullptr) {
        hipError_t e = hipFree(*p);
        *p = nullptr;
        if(e != hipSuccess) {
            return e;
        }
    }
    return hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(count, 1) * sizeof(T));
}

int denoise_ensure(DenoiseWorkspace &ws, size_t n, bool staged) {
    PtDenoiseScratch &d = ws.scratch;
    if(n > ws.pixels) {
        ws.pixels = 0;
        PT_HIP(regrow(&d.col[0], n));
        PT_HIP(regrow(&d.col[1], n));
        PT_HIP(regrow(&d.var[0], n));
        PT_HIP(regrow(&d.var[1], n));
        PT_HIP(regrow(&d.guide, n));
        PT_HIP(regrow(&d.grad, n));
        PT_HIP(regrow(&d.cls, n));
        ws.pixels = n;
    }
    if(staged && n > ws.staged) {
        ws.staged = 0;
        PT_HIP(regrow(&ws.in_rgba, n));
        PT_HIP(regrow(&ws.in_features, 3 * n));
        ws.staged = n;
    }
    return PT_OK;
}

// The parameters pt_denoise takes (NULL = the defaults), checked without a device
int denoise_params_resolve(const pt_denoise_params *params, PtDenoiseParams *resolved) {
    pt_denoise_params p{};
    pt_denoise_params_default(&p);
    if(params != nullptr) {
        p = *params;
    }
    if(p.iterations < 0 || p.iterations > 10) {
        return fail(PT_ERR_INVALID, "iterations must be 0..10");
    }
    for(float sigma : {p.sigma_luminance, p.sigma_normal, p.sigma_depth}) {
        if(!std::isfinite(sigma) || sigma < 0.0F) {
            return fail(PT_ERR_INVALID, "sigmas must be finite and not negative");
        }
    }
    *resolved = PtDenoiseParams{p.iterations, p.sigma_luminance, p.sigma_normal, p.sigma_depth};
    return PT_OK;
}

int denoise_measured_params_resolve(const pt_denoise_measured_params *params, PtDenoiseParams *resolved, float *sigma_measured) {
    pt_denoise_measured_params p{};
    pt_denoise_measured_params_default(&p);
    if(params != nullptr) {
        p = *params;
    }
    PT_TRY(denoise_params_resolve(&p.base, resolved));
    if(!std::isfinite(p.sigma_measured) || p.sigma_measured < 0.0F) {
        return fail(PT_ERR_INVALID, "sigmas must be finite and not negative");
    }
    *sigma_measured = p.sigma_measured;
    return PT_OK;
}

} // namespace pth

// The arguments of the denoise entry points, checked without a device but for its index at the end
static int denoise_views_check(int device, const void *rgba, const void *features, int32_t width, int32_t height, int32_t n_views, const pt_denoise_params *params,
                               const void *out, PtDenoiseParams *resolved) {
    if(n_views <= 0) {
        return fail(PT_ERR_INVALID, "a view batch needs at least one view");
    }
    if(width > 0 && height > 0 && static_cast<uint64_t>(n_views) * static_cast<uint64_t>(width) * static_cast<uint64_t>(height) > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    if(rgba == nullptr || features == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(width <= 0 || height <= 0) {
        return fail(PT_ERR_INVALID, "image size must be positive");
    }
    PtDenoiseParams p{};
    PT_TRY(denoise_params_resolve(params, &p));
    PT_TRY(check_device(device));
    *resolved = p;
    return PT_OK;
}

extern "C" {

int pt_denoise_params_default(pt_denoise_params *out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    out->iterations = 5;
    out->sigma_luminance = 32.0F;
    out->sigma_normal = 128.0F;
    out->sigma_depth = 1.0F;
    return PT_OK;
}

int pt_render_features(pt_scene *s, const pt_camera_params *camera, const pt_options *options, float *out_features) {
    return pt_render_features_views(s, camera, 1, options, out_features);
}

int pt_render_features_device(pt_scene *s, const pt_camera_params *camera, const pt_options *options, float *d_out_features, void *stream) {
    return pt_render_features_views_device(s, camera, 1, options, d_out_features, stream);
}

// pt_render_features_views and its followed form (follow != nullptr: parameters already resolved)
static int render_features_views(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, const pt_feature_params *follow,
                                 float *out_features) {
    const size_t n = static_cast<size_t>(n_views) * static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(s->features.ensure(3 * n));
    PT_TRY(features_views_launch(s, cameras, n_views, options, reinterpret_cast<float4 *>(s->features.ptr), follow));
    PT_HIP(hipMemcpyAsync(out_features, s->features.ptr, 3 * n * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    return PT_OK;
}

static int render_features_views_device(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, const pt_feature_params *follow,
                                        float *d_out_features, void *stream) {
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    // order after the caller's stream, trace on the library's stream, then make the caller's stream wait for it
    StreamOrder order;
    PT_TRY(order.begin(stream, s->stream));
    PT_TRY(features_views_launch(s, cameras, n_views, options, reinterpret_cast<float4 *>(d_out_features), follow));
    PT_TRY(order.end());
    if(order.caller == nullptr) {
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    return PT_OK;
}

int pt_render_features_views(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, float *out_features) {
    PT_TRY(features_views_check(s, cameras, n_views, options, out_features));
    return render_features_views(s, cameras, n_views, options, nullptr, out_features);
}

int pt_render_features_views_device(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, float *d_out_features, void *stream) {
    PT_TRY(features_views_check(s, cameras, n_views, options, d_out_features));
    return render_features_views_device(s, cameras, n_views, options, nullptr, d_out_features, stream);
}

// ---- followed features (include/pt_features.h; pt_walks.hip: pt_follow_kernel) ------------------------------------------------------

int pt_feature_params_default(pt_feature_params *out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    out->max_bounces = 8;
    out->flags = 0;
    return PT_OK;
}

int pt_render_features_followed(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_feature_params *params, float *out_features) {
    return pt_render_features_followed_views(s, camera, 1, options, params, out_features);
}

int pt_render_features_followed_device(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_feature_params *params, float *d_out_features,
                                       void *stream) {
    return pt_render_features_followed_views_device(s, camera, 1, options, params, d_out_features, stream);
}

int pt_render_features_followed_views(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, const pt_feature_params *params,
                                      float *out_features) {
    PT_TRY(features_views_check(s, cameras, n_views, options, out_features));
    pt_feature_params follow{};
    PT_TRY(feature_params_resolve(params, options, &follow));
    return render_features_views(s, cameras, n_views, options, &follow, out_features);
}

int pt_render_features_followed_views_device(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, const pt_feature_params *params,
                                             float *d_out_features, void *stream) {
    PT_TRY(features_views_check(s, cameras, n_views, options, d_out_features));
    pt_feature_params follow{};
    PT_TRY(feature_params_resolve(params, options, &follow));
    return render_features_views_device(s, cameras, n_views, options, &follow, d_out_features, stream);
}

int pt_denoise_device(int device, const float *d_rgba, const float *d_features, int32_t width, int32_t height, const pt_denoise_params *params, float *d_out_rgba,
                      void *stream) {
    return pt_denoise_views_device(device, d_rgba, d_features, width, height, 1, params, d_out_rgba, stream);
}

int pt_denoise(int device, const float *rgba, const float *features, int32_t width, int32_t height, const pt_denoise_params *params, float *out_rgba) {
    return pt_denoise_views(device, rgba, features, width, height, 1, params, out_rgba);
}

// The view forms: n_views frames stacked, every stage one launch for all of them (pt_denoise_views_run; one view: pt_denoise_run itself)
int pt_denoise_views_device(int device, const float *d_rgba, const float *d_features, int32_t width, int32_t height, int32_t n_views, const pt_denoise_params *params,
                            float *d_out_rgba, void *stream) {
    PtDenoiseParams p{};
    PT_TRY(denoise_views_check(device, d_rgba, d_features, width, height, n_views, params, d_out_rgba, &p));
    const size_t n = static_cast<size_t>(n_views) * static_cast<size_t>(width) * static_cast<size_t>(height);
    DenoiseWorkspace &ws = denoise_workspace(device);
    std::lock_guard<std::mutex> lock(ws.mutex);
    PT_HIP(hipSetDevice(device));
    PT_TRY(denoise_ensure(ws, n, false));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PT_HIP(pt_denoise_views_run(st, reinterpret_cast<const float4 *>(d_rgba), reinterpret_cast<const float4 *>(d_features), nullptr, width, height, n_views, p,
                                ws.scratch, reinterpret_cast<float4 *>(d_out_rgba)));
    PT_HIP(hipStreamSynchronize(st)); // the scratch buffers are the device's: the next call may reuse them
    return PT_OK;
}

int pt_denoise_views(int device, const float *rgba, const float *features, int32_t width, int32_t height, int32_t n_views, const pt_denoise_params *params,
                     float *out_rgba) {
    PtDenoiseParams p{};
    PT_TRY(denoise_views_check(device, rgba, features, width, height, n_views, params, out_rgba, &p));
    const size_t n = static_cast<size_t>(n_views) * static_cast<size_t>(width) * static_cast<size_t>(height);
    DenoiseWorkspace &ws = denoise_workspace(device);
    std::lock_guard<std::mutex> lock(ws.mutex);
    PT_HIP(hipSetDevice(device));
    PT_TRY(denoise_ensure(ws, n, true));
    PT_HIP(hipMemcpy(ws.in_rgba, rgba, n * sizeof(F4), hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(ws.in_features, features, 3 * n * sizeof(F4), hipMemcpyHostToDevice));
    // in place: the last kernel reads a pixel's alpha before it writes that pixel, and no kernel reads another pixel of the input
    PT_HIP(pt_denoise_views_run(nullptr, ws.in_rgba, ws.in_features, nullptr, width, height, n_views, p, ws.scratch, ws.in_rgba));
    PT_HIP(hipMemcpy(out_rgba, ws.in_rgba, n * sizeof(F4), hipMemcpyDeviceToHost));
    return PT_OK;
}

// The filter with a plane of measured variances (pt_denoise_measured_run; include/pt_frame_variance.h): mask NULL = the plain filter
static int denoise_measured_check(int device, const void *rgba, const void *features, const void *variance, int32_t width, int32_t height,
                                  const pt_denoise_measured_params *params, const void *out, PtDenoiseParams *resolved, float *sigma_measured) {
    if(rgba == nullptr || features == nullptr || variance == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(width <= 0 || height <= 0) {
        return fail(PT_ERR_INVALID, "image size must be positive");
    }
    if(static_cast<uint64_t>(width) * static_cast<uint64_t>(height) > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    PT_TRY(denoise_measured_params_resolve(params, resolved, sigma_measured));
    return check_device(device);
}

int pt_denoise_measured_params_default(pt_denoise_measured_params *out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    pt_denoise_params_default(&out->base);
    out->sigma_measured = 16.0F;
    return PT_OK;
}

int pt_denoise_measured_device(int device, const float *d_rgba, const float *d_features, const float *d_variance, const int32_t *d_mask, int32_t width,
                               int32_t height, const pt_denoise_measured_params *params, float *d_out_rgba, void *stream) {
    PtDenoiseParams p{};
    float sigma_measured = 0.0F;
    PT_TRY(denoise_measured_check(device, d_rgba, d_features, d_variance, width, height, params, d_out_rgba, &p, &sigma_measured));
    const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
    DenoiseWorkspace &ws = denoise_workspace(device);
    std::lock_guard<std::mutex> lock(ws.mutex);
    PT_HIP(hipSetDevice(device));
    PT_TRY(denoise_ensure(ws, n, false));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PT_HIP(pt_denoise_measured_run(st, reinterpret_cast<const float4 *>(d_rgba), reinterpret_cast<const float4 *>(d_features),
                                   reinterpret_cast<const float4 *>(d_variance), d_mask, width, height, p, sigma_measured, ws.scratch,
                                   reinterpret_cast<float4 *>(d_out_rgba)));
    PT_HIP(hipStreamSynchronize(st)); // the scratch buffers are the device's: the next call may reuse them
    return PT_OK;
}

int pt_denoise_measured(int device, const float *rgba, const float *features, const float *variance, const int32_t *mask, int32_t width, int32_t height,
                        const pt_denoise_measured_params *params, float *out_rgba) {
    PtDenoiseParams p{};
    float sigma_measured = 0.0F;
    PT_TRY(denoise_measured_check(device, rgba, features, variance, width, height, params, out_rgba, &p, &sigma_measured));
    const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
    DenoiseWorkspace &ws = denoise_workspace(device);
    std::lock_guard<std::mutex> lock(ws.mutex);
    PT_HIP(hipSetDevice(device));
    PT_TRY(denoise_ensure(ws, n, true));
    if(n > ws.staged_variance) {
        ws.staged_variance = 0;
        PT_HIP(regrow(&ws.in_variance, n));
        ws.staged_variance = n;
    }
    DevBuf<int32_t> d_mask;
    if(mask != nullptr) {
        PT_HIP(d_mask.ensure(n));
        PT_HIP(hipMemcpy(d_mask.ptr, mask, n * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    PT_HIP(hipMemcpy(ws.in_rgba, rgba, n * sizeof(F4), hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(ws.in_features, features, 3 * n * sizeof(F4), hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(ws.in_variance, variance, n * sizeof(F4), hipMemcpyHostToDevice));
    // in place, as pt_denoise
    PT_HIP(pt_denoise_measured_run(nullptr, ws.in_rgba, ws.in_features, ws.in_variance, mask != nullptr ? d_mask.ptr : nullptr, width, height, p, sigma_measured,
                                   ws.scratch, ws.in_rgba));
    PT_HIP(hipMemcpy(out_rgba, ws.in_rgba, n * sizeof(F4), hipMemcpyDeviceToHost));
    return PT_OK;
}

} // extern "C"

// ---- temporal denoising of a sequence (pt_denoise.hip: pt_temporal_run) ----------------------------------------------------------------

// One sequence's history and scratch, all on `device` and owned by the handle (no shared workspace: two sequences may interleave).
struct pt_temporal {
    int device = 0;
    int32_t width = 0, height = 0;
    PtTemporalParams params{};
    std::mutex mutex;
    DevBuf<float4> col[2], guide, col_hist, pos[2], nrm[2], in_rgba, in_features, in_motion; // (in_motion: pt_temporal_denoise_motion's host form)
    DevBuf<float> var[2];
    DevBuf<float2> grad, moments[2];
    DevBuf<int32_t> len[2];
    DevBuf<uint32_t> cls[2];
    int cur = 0;
    bool has_prev = false;
    PtDevCamera prev{};       // the last push's camera (its basis: all the feature rays depend on) ...
    float prev_rows[3][3] = {}; // ... and its reprojection rows (PtReprojection)
    PtDevCamera pending{};        // the same of the push in flight, until temporal_commit
    float pending_rows[3][3] = {};
};

namespace {

// The basis of `c` (derive_camera), its reprojection rows (PtReprojection) and its pixel footprint for images `height` pixels high;
// PT_ERR_INVALID for a degenerate basis.
int temporal_camera(const pt_camera_params *c, int32_t height, PtDevCamera *cam, float rows[3][3], float *footprint) {
    const float scalars[] = {c->origin[0], c->origin[1], c->origin[2], c->look_at[0], c->look_at[1], c->look_at[2], c->up[0], c->up[1], c->up[2],
                             c->focal_length, c->height, c->aspect_ratio};
    for(float v : scalars) {
        if(!std::isfinite(v)) {
            return fail(PT_ERR_INVALID, "camera: non-finite parameter");
        }
    }
    *cam = derive_camera(c);
    const Vec3 f = ld(cam->forward), u = ld(cam->up), r = ld(cam->right);
    Vec3 row[3] = {cross(u, r), cross(r, f), cross(f, u)}; // the inverse of [f u r], times det
    const float det = dot(f, row[0]);
    if(!std::isfinite(det) || det == 0.0F) {
        return fail(PT_ERR_INVALID, "camera: degenerate basis (look_at = origin, a zero up, height, focal length or aspect ratio, or up along the view)");
    }
    for(int i = 0; i < 3; i++) {
        if(det < 0.0F) { // (a negative aspect ratio): the same ratios, and "in front" stays row[0] . d > 0
            row[i] = scale(row[i], -1.0F);
        }
        const float v[3] = {row[i].x, row[i].y, row[i].z};
        for(int k = 0; k < 3; k++) {
            if(!std::isfinite(v[k])) {
                return fail(PT_ERR_INVALID, "camera: degenerate basis");
            }
            rows[i][k] = v[k];
        }
    }
    *footprint = c->height / (c->focal_length * static_cast<float>(height));
    return PT_OK;
}

int temporal_check_params(const pt_temporal_params &p) {
    if(p.spatial.iterations < 0 || p.spatial.iterations > 10) {
        return fail(PT_ERR_INVALID, "iterations must be 0..10");
    }
    for(float sigma : {p.spatial.sigma_luminance, p.spatial.sigma_normal, p.spatial.sigma_depth, p.sigma_luminance_temporal, p.position_tolerance}) {
        if(!std::isfinite(sigma) || sigma < 0.0F) {
            return fail(PT_ERR_INVALID, "sigmas and position_tolerance must be finite and not negative");
        }
    }
    for(float a : {p.alpha_color, p.alpha_moments}) {
        if(!(a > 0.0F && a <= 1.0F)) {
            return fail(PT_ERR_INVALID, "alphas must be in (0, 1]");
        }
    }
    if(p.max_history < 1 || p.moments_min_history < 1) {
        return fail(PT_ERR_INVALID, "max_history and moments_min_history must be at least 1");
    }
    if(!std::isfinite(p.normal_min)) {
        return fail(PT_ERR_INVALID, "normal_min must be finite");
    }
    return PT_OK;
}

// Checks a push's arguments without touching the handle or a device.
int temporal_check_push(const pt_temporal *t, const void *rgba, const void *features, const pt_camera_params *camera, const void *out) {
    if(t == nullptr || rgba == nullptr || features == nullptr || camera == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    PtDevCamera cam{};
    float rows[3][3];
    float footprint = 0.0F;
    return temporal_camera(camera, 1, &cam, rows, &footprint);
}

// Enqueues one push on `st` (handle mutex held by the caller).  The launch rewrites the colour history, so the handle has no usable history
// until the caller, once every copy of the push's outputs has succeeded, commits the push with temporal_commit; a failure in between leaves
// it with none (its next push starts afresh) rather than pairing this push's camera with the last push's buffers.
// `motion` (may be null: the plain push): the frame's motion in device memory (include/pt_motion.h).
int temporal_push(pt_temporal *t, hipStream_t st, const float4 *rgba, const float4 *features, const float4 *motion, const pt_camera_params *camera, float4 *out) {
    PtReprojection rp{};
    PtDevCamera cam{};
    float rows[3][3];
    PT_TRY(temporal_camera(camera, t->height, &cam, rows, &rp.footprint));
    if(!t->has_prev) {
        rp.mode = PT_REPROJECT_NONE;
    }
    else if(std::memcmp(cam.origin, t->prev.origin, sizeof cam.origin) == 0 && std::memcmp(cam.forward, t->prev.forward, sizeof cam.forward) == 0 &&
            std::memcmp(cam.up, t->prev.up, sizeof cam.up) == 0 && std::memcmp(cam.right, t->prev.right, sizeof cam.right) == 0) {
        rp.mode = PT_REPROJECT_IDENTICAL;
        if(motion != nullptr) { // a pixel on a moved surface is projected under the same camera too
            std::memcpy(rp.origin, t->prev.origin, sizeof rp.origin);
            std::memcpy(rp.row, t->prev_rows, sizeof rp.row);
        }
    }
    else { // into the previous camera
        rp.mode = PT_REPROJECT_CAMERA;
        std::memcpy(rp.origin, t->prev.origin, sizeof rp.origin);
        std::memcpy(rp.row, t->prev_rows, sizeof rp.row);
    }
    PtDenoiseScratch s{};
    s.col[0] = t->col[0].ptr;
    s.col[1] = t->col[1].ptr;
    s.var[0] = t->var[0].ptr;
    s.var[1] = t->var[1].ptr;
    s.guide = t->guide.ptr;
    s.grad = t->grad.ptr;
    PtTemporalState state{};
    state.col_hist = t->col_hist.ptr;
    for(int i = 0; i < 2; i++) {
        state.moments[i] = t->moments[i].ptr;
        state.len[i] = t->len[i].ptr;
        state.pos[i] = t->pos[i].ptr;
        state.nrm[i] = t->nrm[i].ptr;
        state.cls[i] = t->cls[i].ptr;
    }
    state.cur = t->cur;
    t->has_prev = false;
    t->pending = cam;
    std::memcpy(t->pending_rows, rows, sizeof rows);
    if(motion != nullptr) {
        PT_HIP(pt_temporal_run_motion(st, rgba, features, motion, t->width, t->height, t->params, rp, s, state, out));
    }
    else {
        PT_HIP(pt_temporal_run(st, rgba, features, t->width, t->height, t->params, rp, s, state, out));
    }
    return PT_OK;
}

// The push enqueued by temporal_push has completed and its outputs were read: it becomes the history of the next push.
void temporal_commit(pt_temporal *t) {
    t->prev = t->pending;
    std::memcpy(t->prev_rows, t->pending_rows, sizeof t->prev_rows);
    t->has_prev = true;
    t->cur ^= 1;
}

} // namespace

extern "C" {

int pt_temporal_params_default(pt_temporal_params *out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    pt_denoise_params_default(&out->spatial);
    out->alpha_color = 0.2F;
    out->alpha_moments = 0.2F;
    out->max_history = 32;
    out->moments_min_history = 4;
    out->sigma_luminance_temporal = 4.0F;
    out->normal_min = 0.9F;
    out->position_tolerance = 2.0F;
    return PT_OK;
}

int pt_temporal_create(int device, int32_t width, int32_t height, const pt_temporal_params *params, pt_temporal **out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    *out = nullptr;
    if(width <= 0 || height <= 0) {
        return fail(PT_ERR_INVALID, "image size must be positive");
    }
    if(static_cast<long long>(width) * height > 0x0fffffffLL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    pt_temporal_params p{};
    pt_temporal_params_default(&p);
    if(params != nullptr) {
        p = *params;
    }
    PT_TRY(temporal_check_params(p));
    PT_TRY(check_device(device));
    std::unique_ptr<pt_temporal> t(new pt_temporal());
    t->device = device;
    t->width = width;
    t->height = height;
    t->params = PtTemporalParams{PtDenoiseParams{p.spatial.iterations, p.spatial.sigma_luminance, p.spatial.sigma_normal, p.spatial.sigma_depth},
                                 p.alpha_color, p.alpha_moments, p.max_history, p.moments_min_history, p.sigma_luminance_temporal, p.normal_min,
                                 p.position_tolerance};
    const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
    PT_HIP(hipSetDevice(device));
    PT_HIP(t->guide.ensure(n));
    PT_HIP(t->col_hist.ensure(n));
    PT_HIP(t->grad.ensure(n));
    for(int i = 0; i < 2; i++) {
        PT_HIP(t->col[i].ensure(n));
        PT_HIP(t->var[i].ensure(n));
        PT_HIP(t->moments[i].ensure(n));
        PT_HIP(t->len[i].ensure(n));
        PT_HIP(t->pos[i].ensure(n));
        PT_HIP(t->nrm[i].ensure(n));
        PT_HIP(t->cls[i].ensure(n));
    }
    *out = t.release();
    return PT_OK;
}

int pt_temporal_denoise(pt_temporal *t, const float *rgba, const float *features, const pt_camera_params *camera, float *out_rgba, int32_t *out_history) {
    return pt_temporal_denoise_motion(t, rgba, features, nullptr, camera, out_rgba, out_history);
}

int pt_temporal_denoise_motion(pt_temporal *t, const float *rgba, const float *features, const float *motion, const pt_camera_params *camera, float *out_rgba,
                               int32_t *out_history) {
    PT_TRY(temporal_check_push(t, rgba, features, camera, out_rgba));
    std::lock_guard<std::mutex> lock(t->mutex);
    const size_t n = static_cast<size_t>(t->width) * static_cast<size_t>(t->height);
    PT_HIP(hipSetDevice(t->device));
    PT_HIP(t->in_rgba.ensure(n));
    PT_HIP(t->in_features.ensure(3 * n));
    PT_HIP(hipMemcpy(t->in_rgba.ptr, rgba, n * sizeof(float4), hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(t->in_features.ptr, features, 3 * n * sizeof(float4), hipMemcpyHostToDevice));
    if(motion != nullptr) {
        PT_HIP(t->in_motion.ensure(2 * n));
        PT_HIP(hipMemcpy(t->in_motion.ptr, motion, 2 * n * sizeof(float4), hipMemcpyHostToDevice));
    }
    // in place, as pt_denoise
    PT_TRY(temporal_push(t, nullptr, t->in_rgba.ptr, t->in_features.ptr, motion != nullptr ? t->in_motion.ptr : nullptr, camera, t->in_rgba.ptr));
    PT_HIP(hipMemcpy(out_rgba, t->in_rgba.ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
    if(out_history != nullptr) {
        PT_HIP(hipMemcpy(out_history, t->len[t->cur].ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    temporal_commit(t);
    return PT_OK;
}

int pt_temporal_denoise_device(pt_temporal *t, const float *d_rgba, const float *d_features, const pt_camera_params *camera, float *d_out_rgba,
                               int32_t *d_out_history, void *stream) {
    return pt_temporal_denoise_motion_device(t, d_rgba, d_features, nullptr, camera, d_out_rgba, d_out_history, stream);
}

int pt_temporal_denoise_motion_device(pt_temporal *t, const float *d_rgba, const float *d_features, const float *d_motion, const pt_camera_params *camera,
                                      float *d_out_rgba, int32_t *d_out_history, void *stream) {
    PT_TRY(temporal_check_push(t, d_rgba, d_features, camera, d_out_rgba));
    std::lock_guard<std::mutex> lock(t->mutex);
    const size_t n = static_cast<size_t>(t->width) * static_cast<size_t>(t->height);
    PT_HIP(hipSetDevice(t->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PT_TRY(temporal_push(t, st, reinterpret_cast<const float4 *>(d_rgba), reinterpret_cast<const float4 *>(d_features), reinterpret_cast<const float4 *>(d_motion), camera,
                         reinterpret_cast<float4 *>(d_out_rgba)));
    if(d_out_history != nullptr) {
        PT_HIP(hipMemcpyAsync(d_out_history, t->len[t->cur].ptr, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    }
    PT_HIP(hipStreamSynchronize(st));
    temporal_commit(t);
    return PT_OK;
}

int pt_temporal_reset(pt_temporal *t) {
    if(t == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(t->mutex);
    t->has_prev = false;
    return PT_OK;
}

int pt_temporal_destroy(pt_temporal *t) {
    if(t == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    (void)hipSetDevice(t->device);
    delete t;
    return PT_OK;
}

} // extern "C"
