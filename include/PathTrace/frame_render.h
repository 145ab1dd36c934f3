// PathTrace/frame_render.h -- a processJob that can be stopped and continued (an extension of PathTrace/render_control.h).
#ifndef PATHTRACE_FRAME_RENDER_H
#define PATHTRACE_FRAME_RENDER_H

#include <PathTrace/image/image.h>
#include <PathTrace/render_control.h>
#include <PathTrace/worker.h>

#include "../pt_hip.h"

#include <cstdint>
#include <functional>
#include <vector>

// One frame of a FrameRenderJob, rendered in as many calls as the caller likes: every render() continues where the last one stopped
// (its RenderControl's budget ran out or it was cancelled).  The pixels a stop catches half-way park their state on the device and resume
// from it, so no sample is drawn twice, and the finished frame is bit for bit what processJob gives with the same seed
// ($PATHTRACE_SEED, or a random one) on the replicas $PATHTRACE_DEVICES selects -- without denoising: options.allow_bias is ignored (a
// stopped frame has holes: preview() shows one, denoised if asked; denoise the finished frame with PathTrace/denoise.h).  The job's scene
// must outlive the FrameRender.
class FrameRender {
public:
    explicit FrameRender(const FrameRenderJob &job, int worker_count = 0);
    ~FrameRender();
    FrameRender(const FrameRender &) = delete;
    FrameRender &operator=(const FrameRender &) = delete;

    // Continues the frame under `control` (use a fresh control per call: a cancelled control stays cancelled) and returns whether the
    // frame is complete.  control reports the tiles of the whole frame that have finished, and what this call did with its streams
    // (streamsAbandoned: parked for the next call).  Throws std::runtime_error if the device fails; the frame is unusable then.
    bool render(RenderControl &control, const std::function<void(int, int)> &progress_callback = [](int, int) {});
    // the frame so far: finished pixels are final, the others transparent black (0, 0, 0, 0)
    const Image<> &image() const noexcept { return image_; }
    bool complete() const noexcept { return complete_; }
    // where the frame stands (pt_frame_info: streams finished / parked / untouched, tiles, samples the parked streams carry)
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
    // it stands; errorMap(): one rating per pixel, row-major -- -1 finished, +inf unrated or untouched.
    void setNoiseTarget(float target, float floor = 1E-5f, float fraction = 1.0f);
    // The features of the denoised previews (pt_frame_set_feature_params, include/pt_features.h): with parameters they follow mirrors and
    // glass to the first diffuse hit (max_bounces 0..32, flags 0), with null they are the first-hit features again, which is how a frame
    // starts.  The next denoised preview computes its features anew.  Throws std::invalid_argument for parameters outside their range.
    void setFeatureParams(const pt_feature_params *params);
    pt_frame_noise noise() const;
    std::vector<float> errorMap() const;
    bool noiseTargetReached() const;
    // The frame as it stands, for a viewer between two render() calls (pt_frame_preview): finished pixels as image(), parked ones the
    // running mean of their samples so far, untouched ones (0, 0, 0, 0).  `samples` (if not null) gets one count per pixel, row-major:
    // -1 finished, the samples taken of a parked pixel, 0 untouched.  With `denoise` the preview is filtered as pt_denoise filters a frame,
    // holes filled from their neighbours.  out is resized to the frame.  Changes nothing the frame will do.  Throws std::runtime_error on failure.
    void preview(Image<> &out, std::vector<std::int32_t> *samples = nullptr, const pt_denoise_params *denoise = nullptr) const;
    // The measured variance of the unfinished pixels (pt_frame_get_variance, include/pt_frame_variance.h): four floats per pixel, row-major
    // -- the variance of the mean of r, g and b from the estimator's batch statistics and the number of batch means, (0, 0, 0, 0) for a
    // pixel that is finished, untouched or has fewer than two batch means.  previewMeasured(): preview() denoised with each rated pixel's
    // measured variance in place of the filter's 3x3 estimate (pt_frame_preview_measured; params null = pt_denoise_measured_params_default).
    std::vector<float> variance() const;
    void previewMeasured(Image<> &out, std::vector<std::int32_t> *samples = nullptr, const pt_denoise_measured_params *params = nullptr) const;
    std::uint64_t seed() const noexcept { return seed_; }
    // A checkpoint (pt_frame_checkpoint_save / _load, include/pt_checkpoint.h): save() puts the frame as it stands between two render()
    // calls into `blob` (the caller writes it to a file or sends it somewhere); load() makes the frame of such a blob on `scene` -- the
    // scene the frame was made on, built again in this or another process, on any number of device replicas -- with image() holding its
    // finished pixels.  The loaded frame goes on as the saved one would have and finishes bit-identically.  Saving changes nothing.
    // Throw std::runtime_error on failure (a damaged blob, another scene, a view batch's blob: see ViewBatchRender::load).
    void save(std::vector<std::uint8_t> &blob) const;
    static FrameRender load(const Scene &scene, const std::vector<std::uint8_t> &blob, int worker_count = 0) { return FrameRender(scene, blob, worker_count); }

private:
    FrameRender(const Scene &scene, const std::vector<std::uint8_t> &blob, int worker_count);
    Image<> image_;
    std::vector<pt_tile> tiles_;
    pt_frame *frame_ = nullptr;
    std::uint64_t seed_ = 0;
    bool complete_ = false;
};

#endif
