// src/host/worker.cpp -- processItem / processJob of PathTrace/worker.h on top of the C ABI (include/pt_hip.h).
#include <PathTrace/denoise.h>
#include <PathTrace/render_control.h>
#include <PathTrace/worker.h>

#include "../../include/pt_hip.h"
#include "job_params.h"

#include <algorithm>
#include <cstdlib>
#include <exception>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

using namespace pathtrace_host;

WorkItem::WorkItem() noexcept : job(nullptr), offset_x(0), offset_y(0), width(0), height(0) {}

WorkItem::WorkItem(const FrameRenderJob *job, int offset_x, int offset_y, int width, int height) noexcept :
  job(job), offset_x(offset_x), offset_y(offset_y), width(width), height(height) {}

Image<> processItem(const WorkItem &item, RandomEngine &re) {
    Image<> tile(item.width, item.height);
    if(item.width <= 0 || item.height <= 0) {
        return tile;
    }
    const FrameRenderJob &job = *item.job;
    const pt_camera_params camera = cameraParams(job.camera);
    const pt_options options = renderOptions(job.options);
    const pt_stream stream{item.offset_x, item.offset_y, item.width, item.height, re.state()};

    // the device renders into a frame that lives in HBM only; the item's rectangle comes back straight into the tile
    static_assert(sizeof(Color<float>) == 4 * sizeof(float), "Image<Color<float>> is a packed RGBA float array");
    uint64_t state_after = stream.rng_state;
    check(pt_render_item(job.scene.deviceScene(), &camera, &options, &stream, reinterpret_cast<float *>(tile.data()), &state_after, nullptr), "processItem");
    re.setState(state_after);
    return tile;
}

Image<> processJob(const FrameRenderJob &job, const std::function<void(int, int)> &progress_callback, int worker_count) {
    const int width = std::max(job.options.image_width, 0);
    const int height = std::max(job.options.image_height, 0);
    Image<> frame(width, height);
    if(width == 0 || height == 0) {
        return frame;
    }
    const pt_camera_params camera = cameraParams(job.camera);
    const pt_options options = renderOptions(job.options);

    const std::vector<pt_tile> tiles = jobTiles(width, height);
    const uint64_t base_seed = jobSeed();

    // The tiles are dealt to the scene's device replicas ($PATHTRACE_DEVICES; one by default) and rendered by one persistent launch
    // per device.  progress_callback is called as the reference calls it (worker.h:75-78, src/worker.cpp:354-360): once per finished
    // tile, (completed, total), never concurrently -- while the devices are still rendering.
    ForwardProgress forward{&progress_callback, nullptr};
    static_assert(sizeof(Color<float>) == 4 * sizeof(float), "Image<Color<float>> is a packed RGBA float array");
    const std::vector<pt_scene *> &replicas = job.scene.deviceScenes();
    const int status = pt_render_tiles_multi(replicas.data(), replicaCount(replicas, worker_count), &camera, &options, tiles.data(), tiles.size(), base_seed,
                                             reinterpret_cast<float *>(frame.data()), nullptr, &ForwardProgress::call, &forward);
    if(forward.failure) {
        std::rethrow_exception(forward.failure);
    }
    check(status, "processJob");
    if(job.options.allow_bias) {
        // the finished frame, denoised on replica 0 (PathTrace/denoise.h)
        return denoise(frame, job.scene, job.camera, job.options);
    }
    return frame;
}

Image<> processJob(const FrameRenderJob &job, RenderControl &control, const std::function<void(int, int)> &progress_callback, int worker_count) {
    control.cancelled_ = false;
    control.finished_.clear();
    control.tile_count_ = 0;
    const int width = std::max(job.options.image_width, 0);
    const int height = std::max(job.options.image_height, 0);
    Image<> frame(width, height); // (pixels a stop leaves unwritten stay transparent black)
    if(width == 0 || height == 0) {
        return frame;
    }
    const pt_camera_params camera = cameraParams(job.camera);
    const pt_options options = renderOptions(job.options);
    const std::vector<pt_tile> tiles = jobTiles(width, height);
    const uint64_t base_seed = jobSeed();
    ForwardProgress forward{&progress_callback, nullptr};
    std::vector<uint8_t> done(tiles.size(), 0);
    control.ctl_.tile_done = done.data();
    const std::vector<pt_scene *> &replicas = job.scene.deviceScenes();
    const int status = pt_render_tiles_ctl(replicas.data(), replicaCount(replicas, worker_count), &camera, &options, tiles.data(), tiles.size(), base_seed,
                                           reinterpret_cast<float *>(frame.data()), nullptr, &ForwardProgress::call, &forward, &control.ctl_);
    control.ctl_.tile_done = nullptr;
    if(forward.failure) {
        std::rethrow_exception(forward.failure);
    }
    if(status != PT_ERR_CANCELLED) {
        check(status, "processJob");
    }
    control.cancelled_ = status == PT_ERR_CANCELLED;
    control.tile_count_ = tiles.size();
    for(size_t i = 0; i < tiles.size(); i++) {
        if(done[i] != 0) {
            control.finished_.push_back(RenderControl::Tile{tiles[i].x, tiles[i].y, tiles[i].w, tiles[i].h});
        }
    }
    return frame;
}
