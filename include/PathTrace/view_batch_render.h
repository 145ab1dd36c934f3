// PathTrace/view_batch_render.h -- processViews that can be stopped, continued and previewed (PathTrace/view_batch.h and
// PathTrace/frame_render.h together).
#ifndef PATHTRACE_VIEW_BATCH_RENDER_H
#define PATHTRACE_VIEW_BATCH_RENDER_H

#include <PathTrace/camera.h>
#include <PathTrace/image/image.h>
#include <PathTrace/render_control.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

#include "../pt_hip.h"

#include <cstdint>
#include <functional>
#include <vector>

// One frame per camera, all in one launch per device replica as processViews renders them, in as many calls as the caller likes: every
// render() continues where the last one stopped, as FrameRender does for one frame.  The finished images are bit for bit what processViews
// gives with the same $PATHTRACE_SEED (view v takes the seed base + v; pass `seeds` to choose them) -- without denoising: options.allow_bias
// is ignored, preview() shows the batch as it stands, denoised if asked.  A denoised preview of the complete batch equals processViews with
// allow_bias.  The scene must outlive the ViewBatchRender.  Throws std::invalid_argument for an empty camera list, a null camera or a seed
// list of another length.
class ViewBatchRender {
public:
    ViewBatchRender(const Scene &scene, const std::vector<const Camera *> &cameras, const RenderOptions &options, const std::vector<std::uint64_t> &seeds = {},
                    int worker_count = 0);
    ~ViewBatchRender();
    ViewBatchRender(const ViewBatchRender &) = delete;
    ViewBatchRender &operator=(const ViewBatchRender &) = delete;

    // As FrameRender::render; the tiles control reports lie in the stacked image: view v's tiles have y in [v * height, (v + 1) * height).
    bool render(RenderControl &control, const std::function<void(int, int)> &progress_callback = [](int, int) {});
    // the views so far: finished pixels are final, the others transparent black (0, 0, 0, 0)
    std::vector<Image<>> images() const;
    bool complete() const noexcept { return complete_; }
    pt_frame_info info() const;
    // Progressive mode (pt_frame_set_progressive): render() then works in passes, each bringing every unfinished pixel to `quantum` more
    // samples, so that a preview between two calls has samples everywhere; max_passes_per_call > 0 makes render() return (not complete)
    // after that many passes.  quantum 0 turns the mode off.  The finished image does not depend on any of this.  Throws
    // std::invalid_argument for a negative quantum.  progress(): passes completed, the target, the sample counts of the unfinished pixels.
    void setProgressive(int quantum, int max_passes_per_call = 0);
    pt_frame_progress progress() const;
    // A noise target (pt_frame_set_noise_target, include/pt_frame_noise.h): every unfinished pixel is rated by the standard error of its
    // mean, and a progressive frame holds the pixels rated at or below `target` out of its passes; render() returns (not complete) once
    // finished + held pixels are `fraction` of the frame, and noiseTargetReached() is true then.  target 0 clears it: render on, and the
    // finished image is what it always is.  floor keeps dark pixels from dominating (the reference's own is 1E-5).  Throws
    // std::invalid_argument for a negative or non-finite target or floor or a fraction outside (0, 1].  noise(): the summary of the frame as
    // it stands; errorMap(): one rating per pixel, [view][y][x] -- -1 finished, +inf unrated or untouched.
    void setNoiseTarget(float target, float floor = 1E-5f, float fraction = 1.0f);
    // The features of the denoised previews (pt_frame_set_feature_params, include/pt_features.h): with parameters they follow mirrors and
    // glass to the first diffuse hit (max_bounces 0..32, flags 0), with null they are the first-hit features again, which is how a frame
    // starts.  The next denoised preview computes its features anew.  Throws std::invalid_argument for parameters outside their range.
    void setFeatureParams(const pt_feature_params *params);
    pt_frame_noise noise() const;
    std::vector<float> errorMap() const;
    bool noiseTargetReached() const;
    // As FrameRender::preview, per view: `out` gets one image per view, `samples` (if not null) one count per pixel, [view][y][x].  With
    // `denoise` a hole is filled from pixels of its own view only.
    void preview(std::vector<Image<>> &out, std::vector<std::int32_t> *samples = nullptr, const pt_denoise_params *denoise = nullptr) const;
    const std::vector<std::uint64_t> &seeds() const noexcept { return seeds_; }
    std::size_t viewCount() const noexcept { return seeds_.size(); }
    // A checkpoint, as FrameRender::save and FrameRender::load: of the whole batch.  load() throws std::runtime_error for the blob of a
    // single frame (FrameRender::load takes it).
    void save(std::vector<std::uint8_t> &blob) const;
    static ViewBatchRender load(const Scene &scene, const std::vector<std::uint8_t> &blob, int worker_count = 0) { return ViewBatchRender(scene, blob, worker_count); }

private:
    ViewBatchRender(const Scene &scene, const std::vector<std::uint8_t> &blob, int worker_count);
    std::vector<Image<>> split(const std::vector<float> &stacked) const;

    int width_ = 0, height_ = 0;
    std::vector<float> stacked_; // [V][H][W][4]
    std::vector<pt_tile> tiles_;
    std::vector<std::uint64_t> seeds_;
    pt_frame *frame_ = nullptr;
    bool complete_ = false;
};

#endif
