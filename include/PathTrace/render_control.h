// PathTrace/render_control.h -- processJob that can be cancelled or given a time budget (an extension of PathTrace/worker.h).
#ifndef PATHTRACE_RENDER_CONTROL_H
#define PATHTRACE_RENDER_CONTROL_H

#include <PathTrace/image/image.h>
#include <PathTrace/worker.h>

#include "../pt_hip.h"

#include <chrono>
#include <cstdint>
#include <functional>
#include <vector>

// The stop and the outcome of one controlled processJob.  The stop is cooperative: the device drops its streams at their next sample
// boundary, and a pixel is only written once it has finished, so every pixel of a finished tile is exactly what processJob gives with
// the same seed.  One control serves one render at a time; cancel() may be called from the progress callback or from any other thread.
// A control stays cancelled once cancel() has been called: a new render needs a new control.
class RenderControl {
public:
    struct Tile {
        int offset_x, offset_y, width, height;
    };

    RenderControl() noexcept : ctl_{} {}
    RenderControl(const RenderControl &) = delete;
    RenderControl &operator=(const RenderControl &) = delete;

    // thread-safe, non-blocking
    void cancel() noexcept { pt_render_cancel(&ctl_); }
    // wall-clock budget counted from the start of processJob; zero or less = none
    void setBudget(std::chrono::duration<double, std::milli> budget) noexcept { ctl_.budget_ms = budget.count(); }

    // outcome of the last processJob with this control
    bool cancelled() const noexcept { return cancelled_; } // stopped before every tile had finished
    const std::vector<Tile> &finishedTiles() const noexcept { return finished_; }
    std::size_t tileCount() const noexcept { return tile_count_; }
    std::uint64_t streamsFinished() const noexcept { return ctl_.streams_finished; }
    std::uint64_t streamsAbandoned() const noexcept { return ctl_.streams_abandoned; }
    std::uint64_t streamsUnclaimed() const noexcept { return ctl_.streams_unclaimed; }
    double drainMilliseconds() const noexcept { return ctl_.drain_ms; }

private:
    friend Image<> processJob(const FrameRenderJob &, RenderControl &, const std::function<void(int, int)> &, int);
    friend class FrameRender; // (PathTrace/frame_render.h: a resumable processJob)
    friend class ViewBatchRender; // (PathTrace/view_batch_render.h: a resumable processViews)
    pt_render_control ctl_;
    bool cancelled_ = false;
    std::vector<Tile> finished_;
    std::size_t tile_count_ = 0;
};

// processJob (PathTrace/worker.h) under a RenderControl: the same tiles, seeding, device replicas and progress reports.  It returns
// normally when stopped; then control.cancelled() is true, the pixels of control.finishedTiles() are final and the others are transparent
// black (0, 0, 0, 0) -- or partly final, if a tile was stopped halfway.  options.allow_bias is ignored: a stopped frame has holes, and is
// never denoised.  Throws std::runtime_error if the device fails.
Image<> processJob(
  const FrameRenderJob &job, RenderControl &control, const std::function<void(int, int)> &progress_callback = [](int, int) {}, int worker_count = 0);

#endif
