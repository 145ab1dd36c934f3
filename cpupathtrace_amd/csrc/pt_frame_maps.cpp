// pt_frame_maps.cpp -- the maps of an unfinished frame (pt_frames.h): its preview (pt_frame_preview, pt_frame_preview_measured), its noise
// (pt_frame_get_noise; include/pt_frame_noise.h) and its variance (pt_frame_get_variance; include/pt_frame_variance.h).
//
// Every map is made in two steps.  Step 1 (map_gather): each replica that has rendered turns its work list into compact entries on its
// own device, with the map's kernel of pt_frame.hip, and the entries of every replica but 0 come to the host.  Step 2 (map_compose), on
// replica 0's device: the map's base is laid down, and every replica's entries are scattered over it, the far ones by way of one pair of
// staging buffers.  A map passes in which pt_frame::Entries it keeps, its two kernels and its base.
#include "pt_frames.h"

#include <limits>

using namespace pth;

namespace {

typedef pt_frame::Replica Replica;
typedef pt_frame::Entries Entries;

// What step 1 brought to the host, per replica (empty: nothing came): its entries, the second array behind the first, and its summary
struct FarEntries {
    std::vector<std::vector<uint8_t>> entries;
    std::vector<std::vector<uint32_t>> summary;
    explicit FarEntries(const pt_frame *f) : entries(f->reps.size()), summary(f->reps.size()) {}
};

// What every map's entry point does first: the frame's pixel count `n`, its lock, its status, and whether any replica has rendered (before
// the first pt_frame_render no pixel has been touched, and the map says so without a device)
int map_enter(const pt_frame *f, std::unique_lock<std::mutex> &lock, size_t *n, bool *any_ready) {
    // (a view frame's image is its views stacked: a map sees one frame of rows() rows)
    *n = static_cast<size_t>(f->options.image_width) * static_cast<size_t>(f->rows());
    if(*n > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    lock = std::unique_lock<std::mutex>(f->mutex);
    PT_TRY(f->check());
    *any_ready = false;
    for(const auto &r : f->reps) {
        *any_ready = *any_ready || r->ready;
    }
    return PT_OK;
}

// Step 1: launch(r, m) enqueues the map's kernel over replica r's work list into m = r.*map on r's stream and returns what the launch
// wrapper returns (`what`: the message when that is a failure).  ms: null, or where the device time of the kernels is summed up.  The
// summary always comes to the host, the entries of a replica other than 0 when `bring`; a replica's stream is synchronised when
// something came from it or its kernel was timed -- else the stream orders the kernel before step 2.
template<typename Launch>
int map_gather(pt_frame *f, Entries Replica::*map, bool bring, double *ms, FarEntries &far, const Launch &launch, const char *what) {
    if(ms != nullptr) {
        *ms = 0.0;
    }
    for(size_t i = 0; i < f->reps.size(); i++) {
        Replica &r = *f->reps[i];
        if(!r.ready || r.n_todo == 0) {
            continue;
        }
        pt_scene *s = r.s;
        std::lock_guard<std::mutex> lock(s->render_mutex);
        PT_HIP(hipSetDevice(s->device));
        r.previewed = true;
        Entries &m = r.*map;
        const size_t bytes[2] = {r.n_todo * m.size[0], r.n_todo * m.size[1]};
        PT_HIP(m.own[0].ensure(bytes[0]));
        if(bytes[1] != 0) {
            PT_HIP(m.own[1].ensure(bytes[1]));
        }
        if(m.summary_words != 0) {
            PT_HIP(m.summary.ensure(m.summary_words));
        }
        EventPair timer;
        if(ms != nullptr) {
            PT_HIP(timer.begin(s->stream));
        }
        PT_LAUNCH(launch(r, m), what);
        if(ms != nullptr) {
            PT_HIP(timer.end(s->stream));
        }
        bool came = false;
        if(m.summary_words != 0) {
            far.summary[i].resize(m.summary_words);
            PT_HIP(hipMemcpyAsync(far.summary[i].data(), m.summary.ptr, m.summary_words * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
            came = true;
        }
        if(bring && i != 0) {
            far.entries[i].resize(bytes[0] + bytes[1]);
            PT_HIP(hipMemcpyAsync(far.entries[i].data(), m.own[0].ptr, bytes[0], hipMemcpyDeviceToHost, s->stream));
            if(bytes[1] != 0) {
                PT_HIP(hipMemcpyAsync(far.entries[i].data() + bytes[0], m.own[1].ptr, bytes[1], hipMemcpyDeviceToHost, s->stream));
            }
            came = true;
        }
        if(came || ms != nullptr) {
            PT_HIP(hipStreamSynchronize(s->stream));
        }
        if(ms != nullptr) {
            float t = 0.0f;
            PT_HIP(timer.ms(&t));
            *ms += t;
        }
    }
    return PT_OK;
}

// Step 2, on replica 0's device (its render_mutex held; the caller has sized the map, set r0.previewed and enqueued the base on its
// stream): scatter(stream, n, a, b) enqueues the map's scatter of n entries in the arrays a and b, as launch does in step 1.  Replica
// 0's own entries are where step 1 left them; the others pass through the staging buffers, one replica after the other in stream order.
template<typename Scatter>
int map_compose(pt_frame *f, Entries Replica::*map, const FarEntries &far, const Scatter &scatter, const char *what) {
    Replica &r0 = *f->reps[0];
    Entries &m = r0.*map;
    hipStream_t st = r0.s->stream;
    for(size_t i = 0; i < f->reps.size(); i++) {
        const Replica &r = *f->reps[i];
        if(!r.ready || r.n_todo == 0) {
            continue;
        }
        const void *at[2] = {m.own[0].ptr, m.own[1].ptr};
        if(i != 0) {
            const size_t bytes[2] = {r.n_todo * m.size[0], r.n_todo * m.size[1]};
            PT_HIP(m.stage[0].ensure(bytes[0]));
            if(bytes[1] != 0) {
                PT_HIP(m.stage[1].ensure(bytes[1]));
            }
            PT_HIP(hipMemcpyAsync(m.stage[0].ptr, far.entries[i].data(), bytes[0], hipMemcpyHostToDevice, st));
            if(bytes[1] != 0) {
                PT_HIP(hipMemcpyAsync(m.stage[1].ptr, far.entries[i].data() + bytes[0], bytes[1], hipMemcpyHostToDevice, st));
            }
            at[0] = m.stage[0].ptr;
            at[1] = m.stage[1].ptr;
        }
        PT_LAUNCH(scatter(st, r.n_todo, at[0], at[1]), what);
    }
    return PT_OK;
}

// Which pixels a tile of the frame covers, on replica 0's device (its render_mutex held), for the bases of the preview and of the error
// map; built once.  Both bases mean "a tile whose replica has rendered".  Where they are laid down that is every tile: some replica is
// ready and the frame has not failed, the frame's first round launches every replica that has tiles, a launch makes its replica ready
// before anything can stop it (frame_prepare), and a launch that fails before that fails the frame for good.
int frame_cover(pt_frame *f, size_t n) {
    Replica &r0 = *f->reps[0];
    if(r0.cover_ready) {
        return PT_OK;
    }
    const int32_t width = f->options.image_width;
    std::vector<uint8_t> cover(n, 0);
    for(const pt_tile &t : f->tiles) {
        for(int32_t y = t.y; y < t.y + t.h; y++) {
            std::memset(cover.data() + static_cast<size_t>(y) * width + t.x, 1, static_cast<size_t>(t.w));
        }
    }
    PT_HIP(r0.cover.upload(cover));
    r0.cover_ready = true;
    return PT_OK;
}

// The variance map, step 1: pixel_variance of every entry and its pixel
int variance_gather(pt_frame *f, FarEntries &far) {
    PtDevOptions opt;
    PT_TRY(derive_options(&f->options, &opt));
    return map_gather(f, &Replica::variance, true, &f->variance_gather_ms, far, [&](Replica &r, Entries &m) {
        return pt_launch_frame_variance(r.s->stream, r.d_todo[r.cur].ptr, r.n_todo, r.d_park[r.pcur].ptr, r.d_tiles.ptr, r.d_offset.ptr, static_cast<uint32_t>(r.tiles.size()),
                                        f->options.image_width, opt, reinterpret_cast<float4 *>(m.own[0].ptr), reinterpret_cast<int32_t *>(m.own[1].ptr));
    }, "variance: gather kernel failed to launch");
}

// ... and step 2: the map of n pixels in r0.vr_map.  The base is zeros: finished, untouched and uncovered pixels are (0, 0, 0, 0).
int variance_compose(pt_frame *f, size_t n, const FarEntries &far) {
    Replica &r0 = *f->reps[0];
    r0.previewed = true;
    PT_HIP(r0.vr_map.ensure(n));
    PT_HIP(hipMemsetAsync(r0.vr_map.ptr, 0, n * sizeof(F4), r0.s->stream));
    return map_compose(f, &Replica::variance, far, [&](hipStream_t st, uint32_t count, const void *var, const void *at) {
        return pt_launch_frame_variance_scatter(st, static_cast<const float4 *>(var), static_cast<const int32_t *>(at), count, reinterpret_cast<float4 *>(r0.vr_map.ptr));
    }, "variance: scatter kernel failed to launch");
}

// pt_frame_preview (sigma_measured == nullptr) and pt_frame_preview_measured: `dp` is the filter's parameters when `denoise`
int frame_preview(pt_frame *f, const float *image, bool denoise, const PtDenoiseParams &dp, const float *sigma_measured, float *out_rgba, int32_t *out_samples) {
    const int32_t width = f->options.image_width, height = f->options.image_height;
    std::unique_lock<std::mutex> frame_lock;
    size_t n = 0;
    bool any_ready = false;
    PT_TRY(map_enter(f, frame_lock, &n, &any_ready));
    if(!any_ready) {
        // every pixel is a hole, and a frame of holes stays one when it is filtered
        std::memset(out_rgba, 0, n * sizeof(F4));
        if(out_samples != nullptr) {
            std::memset(out_samples, 0, n * sizeof(int32_t));
        }
        return PT_OK;
    }
    // 1. the entries: the running mean of a parked stream and (pixel, samples); for the measured preview also the variances
    FarEntries far(f), far_var(f);
    PT_TRY(map_gather(f, &Replica::preview, true, nullptr, far, [&](Replica &r, Entries &m) {
        return pt_launch_frame_gather(r.s->stream, r.d_todo[r.cur].ptr, r.n_todo, r.n_parked, r.d_park[r.pcur].ptr, r.d_tiles.ptr, r.d_offset.ptr,
                                      static_cast<uint32_t>(r.tiles.size()), width, reinterpret_cast<float4 *>(m.own[0].ptr), reinterpret_cast<int2 *>(m.own[1].ptr));
    }, "preview: gather kernel failed to launch"));
    if(sigma_measured != nullptr) {
        PT_TRY(variance_gather(f, far_var));
    }
    Replica &r0 = *f->reps[0];
    pt_scene *s0 = r0.s;
    std::lock_guard<std::mutex> lock(s0->render_mutex);
    PT_HIP(hipSetDevice(s0->device));
    hipStream_t st = s0->stream;
    // 2. the view of n pixels in r0.pv_view, its sample counts in r0.pv_samples: the caller's image, finished (-1) where a tile covers
    // the pixel and a hole elsewhere, every replica's entries over them
    r0.previewed = true;
    PT_HIP(r0.pv_view.ensure(n));
    PT_HIP(r0.pv_samples.ensure(n));
    PT_TRY(frame_cover(f, n));
    float4 *view = reinterpret_cast<float4 *>(r0.pv_view.ptr);
    PT_HIP(hipMemcpyAsync(view, image, n * sizeof(F4), hipMemcpyHostToDevice, st));
    PT_LAUNCH(pt_launch_frame_preview_base(st, view, r0.pv_samples.ptr, r0.cover.ptr, static_cast<uint32_t>(n)), "preview: base kernel failed to launch");
    PT_TRY(map_compose(f, &Replica::preview, far, [&](hipStream_t stream, uint32_t count, const void *rgba, const void *at) {
        return pt_launch_frame_scatter(stream, static_cast<const float4 *>(rgba), static_cast<const int2 *>(at), count, view, r0.pv_samples.ptr);
    }, "preview: scatter kernel failed to launch"));
    // 3. the filter, and the view back to the caller
    std::unique_lock<std::mutex> ws_lock;
    EventPair timer;
    if(denoise) {
        if(!r0.pv_features_ready) {
            PT_HIP(r0.pv_features.ensure(3 * n));
            PT_TRY(features_views_launch(s0, f->n_views > 1 ? f->cameras.data() : &f->camera, f->n_views, &f->options, reinterpret_cast<float4 *>(r0.pv_features.ptr),
                                         f->follow_features ? &f->feature_params : nullptr));
            r0.pv_features_ready = true;
        }
        DenoiseWorkspace &ws = denoise_workspace(s0->device);
        ws_lock = std::unique_lock<std::mutex>(ws.mutex); // (held until the stream has been synchronised below)
        PT_TRY(denoise_ensure(ws, n, false));
        // (one view: pt_denoise_masked_run itself; more: its view form, a hole filled from its own view only)
        if(sigma_measured != nullptr) {
            PT_TRY(variance_compose(f, n, far_var));
        }
        PT_HIP(timer.begin(st));
        if(sigma_measured != nullptr) {
            PT_HIP(pt_denoise_measured_run(st, view, reinterpret_cast<const float4 *>(r0.pv_features.ptr), reinterpret_cast<const float4 *>(r0.vr_map.ptr),
                                           r0.pv_samples.ptr, width, height, dp, *sigma_measured, ws.scratch, view));
        }
        else {
            PT_HIP(pt_denoise_views_run(st, view, reinterpret_cast<const float4 *>(r0.pv_features.ptr), r0.pv_samples.ptr, width, height, f->n_views, dp, ws.scratch, view));
        }
        PT_HIP(timer.end(st));
    }
    PT_HIP(hipMemcpyAsync(out_rgba, view, n * sizeof(F4), hipMemcpyDeviceToHost, st));
    if(out_samples != nullptr) {
        PT_HIP(hipMemcpyAsync(out_samples, r0.pv_samples.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    PT_HIP(hipStreamSynchronize(st));
    if(denoise) {
        float ms = 0.0f;
        PT_HIP(timer.ms(&ms));
        f->preview_filter_ms = ms;
    }
    return PT_OK;
}

} // namespace

extern "C" {

int pt_frame_preview(pt_frame *f, const float *image, const pt_denoise_params *denoise, float *out_rgba, int32_t *out_samples) {
    if(f == nullptr || image == nullptr || out_rgba == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    PtDenoiseParams dp{};
    if(denoise != nullptr) {
        PT_TRY(denoise_params_resolve(denoise, &dp));
    }
    return frame_preview(f, image, denoise != nullptr, dp, nullptr, out_rgba, out_samples);
}

int pt_frame_preview_measured(pt_frame *f, const float *image, const pt_denoise_measured_params *params, float *out_rgba, int32_t *out_samples) {
    if(f == nullptr || image == nullptr || out_rgba == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    PtDenoiseParams dp{};
    float sigma_measured = 0.0f;
    PT_TRY(denoise_measured_params_resolve(params, &dp, &sigma_measured));
    if(f->n_views > 1) {
        return fail(PT_ERR_UNSUPPORTED, "a view frame has no measured preview");
    }
    return frame_preview(f, image, true, dp, &sigma_measured, out_rgba, out_samples);
}

int pt_frame_get_noise(pt_frame *f, pt_frame_noise *out, float *out_error) {
    if(f == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::unique_lock<std::mutex> frame_lock;
    size_t n = 0;
    bool any_ready = false;
    PT_TRY(map_enter(f, frame_lock, &n, &any_ready));
    PtDevOptions opt;
    PT_TRY(derive_options(&f->options, &opt));
    const PtNoiseRule rule = f->noise_rule(opt, true);
    // 1. the entries, (pixel, bits of its error), wanted with a map only, and every replica's summary
    FarEntries far(f);
    PT_TRY(map_gather(f, &Replica::noise, out_error != nullptr, &f->noise_rate_ms, far, [&](Replica &r, Entries &m) {
        return pt_launch_frame_rate(r.s->stream, r.d_todo[r.cur].ptr, r.n_todo, r.d_park[r.pcur].ptr, r.d_tiles.ptr, r.d_offset.ptr, static_cast<uint32_t>(r.tiles.size()),
                                    f->options.image_width, rule, reinterpret_cast<uint2 *>(m.own[0].ptr), m.summary.ptr);
    }, "noise: rating kernel failed to launch"));
    std::memset(out, 0, sizeof(*out));
    out->target_error = f->noise_target;
    out->floor = f->noise_floor;
    out->fraction = f->noise_fraction;
    out->streams_total = f->streams_total;
    uint32_t max_bits = 0;
    uint64_t left = 0;
    for(size_t i = 0; i < f->reps.size(); i++) {
        const Replica &r = *f->reps[i];
        const std::vector<uint32_t> &summary = far.summary[i];
        left += r.n_todo;
        if(summary.empty()) {
            out->streams_unrated += r.n_todo; // (no launch yet: its streams are untouched)
            continue;
        }
        out->streams_rated += summary[PT_NOISE_RATED];
        out->streams_unrated += summary[PT_NOISE_UNRATED];
        out->streams_held += summary[PT_NOISE_HELD];
        max_bits = std::max(max_bits, summary[PT_NOISE_MAX_BITS]);
        for(int b = 0; b < 64; b++) {
            out->histogram[b] += summary[PT_NOISE_FIRST_BIN + b];
        }
    }
    out->streams_finished = f->streams_total - left;
    out->max_error = from_bits(max_bits);
    out->target_reached = f->noise_target > 0.0f && static_cast<double>(out->streams_finished + out->streams_held) >=
                                                       static_cast<double>(f->noise_fraction) * static_cast<double>(f->streams_total)
                            ? 1
                            : 0;
    if(out_error == nullptr) {
        return PT_OK;
    }
    if(!any_ready) {
        std::fill(out_error, out_error + n, std::numeric_limits<float>::infinity()); // (every pixel is untouched)
        return PT_OK;
    }
    // 2. the map of n pixels in r0.nz_map: finished (-1) where a tile covers the pixel, +inf elsewhere, every replica's entries over them
    Replica &r0 = *f->reps[0];
    pt_scene *s0 = r0.s;
    std::lock_guard<std::mutex> lock(s0->render_mutex);
    PT_HIP(hipSetDevice(s0->device));
    r0.previewed = true;
    PT_HIP(r0.nz_map.ensure(n));
    PT_TRY(frame_cover(f, n));
    PT_LAUNCH(pt_launch_frame_noise_base(s0->stream, r0.nz_map.ptr, r0.cover.ptr, static_cast<uint32_t>(n)), "noise: base kernel failed to launch");
    PT_TRY(map_compose(f, &Replica::noise, far, [&](hipStream_t st, uint32_t count, const void *rated, const void *) {
        return pt_launch_frame_noise_scatter(st, static_cast<const uint2 *>(rated), count, r0.nz_map.ptr);
    }, "noise: scatter kernel failed to launch"));
    PT_HIP(hipMemcpyAsync(out_error, r0.nz_map.ptr, n * sizeof(float), hipMemcpyDeviceToHost, s0->stream));
    PT_HIP(hipStreamSynchronize(s0->stream));
    return PT_OK;
}

int pt_frame_get_variance(pt_frame *f, float *out_var) {
    if(f == nullptr || out_var == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::unique_lock<std::mutex> frame_lock;
    size_t n = 0;
    bool any_ready = false;
    PT_TRY(map_enter(f, frame_lock, &n, &any_ready));
    if(!any_ready) {
        std::memset(out_var, 0, n * sizeof(F4)); // (every pixel is untouched)
        return PT_OK;
    }
    FarEntries far(f);
    PT_TRY(variance_gather(f, far));
    pt_scene *s0 = f->reps[0]->s;
    std::lock_guard<std::mutex> lock(s0->render_mutex);
    PT_HIP(hipSetDevice(s0->device));
    PT_TRY(variance_compose(f, n, far));
    PT_HIP(hipMemcpyAsync(out_var, f->reps[0]->vr_map.ptr, n * sizeof(F4), hipMemcpyDeviceToHost, s0->stream));
    PT_HIP(hipStreamSynchronize(s0->stream));
    return PT_OK;
}

// diagnostic (tools/noise_probe.py): the device time of the rating kernels of the frame's last pt_frame_get_noise, all replicas
int pt_debug_frame_noise_ms(pt_frame *f, double *out_ms) {
    if(f == nullptr || out_ms == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    *out_ms = f->noise_rate_ms;
    return PT_OK;
}

// diagnostic (tools/measured_probe.py): the device time of the gather kernels of the frame's last variance map, all replicas, and of the
// filter of its last denoised preview (either may be NULL)
int pt_debug_frame_measured_ms(pt_frame *f, double *out_gather_ms, double *out_filter_ms) {
    if(f == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    if(out_gather_ms != nullptr) {
        *out_gather_ms = f->variance_gather_ms;
    }
    if(out_filter_ms != nullptr) {
        *out_filter_ms = f->preview_filter_ms;
    }
    return PT_OK;
}

} // extern "C"
