// src/host/view_batch_render.cpp -- ViewBatchRender of PathTrace/view_batch_render.h on top of pt_frame_create_views (include/pt_hip.h).
#include <PathTrace/view_batch_render.h>

#include "../../include/pt_hip.h"
#include "job_params.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <vector>

using namespace pathtrace_host;

ViewBatchRender::ViewBatchRender(const Scene &scene, const std::vector<const Camera *> &cameras, const RenderOptions &options, const std::vector<std::uint64_t> &seeds,
                                 int worker_count) :
  width_(std::max(options.image_width, 0)), height_(std::max(options.image_height, 0)) {
    if(cameras.empty()) {
        throw std::invalid_argument("PathTrace: ViewBatchRender needs at least one camera");
    }
    if(!seeds.empty() && seeds.size() != cameras.size()) {
        throw std::invalid_argument("PathTrace: ViewBatchRender needs one seed per camera");
    }
    std::vector<pt_camera_params> params;
    params.reserve(cameras.size());
    for(const Camera *camera : cameras) {
        if(camera == nullptr) {
            throw std::invalid_argument("PathTrace: ViewBatchRender got a null camera");
        }
        params.push_back(cameraParams(*camera));
    }
    seeds_ = seeds.empty() ? viewSeeds(cameras.size()) : seeds;
    if(width_ == 0 || height_ == 0) {
        complete_ = true;
        return;
    }
    stacked_.assign(static_cast<size_t>(width_) * static_cast<size_t>(height_) * 4 * cameras.size(), 0.0F);
    // the frame's tile list: every view's jobTiles, moved down by v * height
    const std::vector<pt_tile> per_view = jobTiles(width_, height_);
    for(size_t v = 0; v < cameras.size(); v++) {
        for(pt_tile t : per_view) {
            t.y += static_cast<int32_t>(v) * height_;
            tiles_.push_back(t);
        }
    }
    const pt_options opt = renderOptions(options);
    const std::vector<pt_scene *> &replicas = scene.deviceScenes();
    check(pt_frame_create_views(replicas.data(), replicaCount(replicas, worker_count), params.data(), seeds_.data(), static_cast<int32_t>(cameras.size()), &opt, &frame_),
          "ViewBatchRender");
}

// ViewBatchRender::load
ViewBatchRender::ViewBatchRender(const Scene &scene, const std::vector<std::uint8_t> &blob, int worker_count) {
    pt_checkpoint_info info{};
    check(pt_checkpoint_inspect(blob.data(), blob.size(), &info), "ViewBatchRender::load");
    if(info.n_views < 2) {
        throw std::runtime_error("PathTrace: ViewBatchRender::load: the checkpoint is of a single frame (FrameRender::load takes it)");
    }
    width_ = info.options.image_width;
    height_ = info.options.image_height;
    const size_t views = static_cast<size_t>(info.n_views);
    seeds_.resize(views);
    const size_t tables = sizeof(pt_checkpoint_header);
    std::memcpy(seeds_.data(), blob.data() + (tables + views * sizeof(pt_camera_params) + 15) / 16 * 16, views * sizeof(std::uint64_t));
    tiles_.resize(static_cast<size_t>(info.n_tiles));
    std::memcpy(tiles_.data(), blob.data() + (tables + info.bytes_tables + 15) / 16 * 16, tiles_.size() * sizeof(pt_tile));
    stacked_.assign(static_cast<size_t>(width_) * static_cast<size_t>(height_) * 4 * views, 0.0F);
    const std::vector<pt_scene *> &replicas = scene.deviceScenes();
    check(pt_frame_checkpoint_load(replicas.data(), replicaCount(replicas, worker_count), blob.data(), blob.size(), stacked_.data(), &frame_), "ViewBatchRender::load");
    complete_ = info.streams_finished == info.n_streams;
}

void ViewBatchRender::save(std::vector<std::uint8_t> &blob) const {
    blob.clear();
    if(frame_ == nullptr) {
        return; // (a batch without pixels has nothing to save)
    }
    size_t bytes = 0;
    check(pt_frame_checkpoint_size(frame_, &bytes), "ViewBatchRender::save");
    blob.resize(bytes);
    check(pt_frame_checkpoint_save(frame_, stacked_.data(), blob.data(), blob.size(), &bytes), "ViewBatchRender::save");
    blob.resize(bytes);
}

ViewBatchRender::~ViewBatchRender() {
    if(frame_ != nullptr) {
        pt_frame_destroy(frame_);
    }
}

bool ViewBatchRender::render(RenderControl &control, const std::function<void(int, int)> &progress_callback) {
    control.cancelled_ = false;
    control.finished_.clear();
    control.tile_count_ = tiles_.size();
    if(frame_ == nullptr) {
        return complete_;
    }
    ForwardProgress forward{&progress_callback, nullptr};
    std::vector<uint8_t> done(tiles_.size(), 0);
    control.ctl_.tile_done = done.data();
    const int status = pt_frame_render(frame_, stacked_.data(), nullptr, &ForwardProgress::call, &forward, &control.ctl_);
    control.ctl_.tile_done = nullptr;
    if(forward.failure) {
        std::rethrow_exception(forward.failure);
    }
    if(status != PT_ERR_CANCELLED) {
        check(status, "ViewBatchRender::render");
    }
    control.cancelled_ = status == PT_ERR_CANCELLED;
    for(size_t i = 0; i < tiles_.size(); i++) {
        if(done[i] != 0) {
            control.finished_.push_back(RenderControl::Tile{tiles_[i].x, tiles_[i].y, tiles_[i].w, tiles_[i].h});
        }
    }
    complete_ = status == PT_OK;
    return complete_;
}

std::vector<Image<>> ViewBatchRender::split(const std::vector<float> &stacked) const {
    static_assert(sizeof(Color<float>) == 4 * sizeof(float), "Image<Color<float>> is a packed RGBA float array");
    const size_t per_view = static_cast<size_t>(width_) * static_cast<size_t>(height_);
    std::vector<Image<>> views;
    views.reserve(seeds_.size());
    for(size_t v = 0; v < seeds_.size(); v++) {
        views.emplace_back(width_, height_);
        if(per_view > 0 && !stacked.empty()) {
            std::memcpy(views[v].data(), stacked.data() + v * per_view * 4, per_view * 4 * sizeof(float));
        }
    }
    return views;
}

std::vector<Image<>> ViewBatchRender::images() const {
    return split(stacked_);
}

pt_frame_info ViewBatchRender::info() const {
    pt_frame_info i{};
    if(frame_ != nullptr) {
        check(pt_frame_get_info(frame_, &i), "ViewBatchRender::info");
    }
    return i;
}

void ViewBatchRender::setProgressive(int quantum, int max_passes_per_call) {
    if(quantum < 0) {
        throw std::invalid_argument("ViewBatchRender::setProgressive: negative quantum");
    }
    if(frame_ != nullptr) {
        check(pt_frame_set_progressive(frame_, quantum, max_passes_per_call), "ViewBatchRender::setProgressive");
    }
}

pt_frame_progress ViewBatchRender::progress() const {
    pt_frame_progress p{};
    if(frame_ != nullptr) {
        check(pt_frame_get_progress(frame_, &p), "ViewBatchRender::progress");
    }
    return p;
}

void ViewBatchRender::setFeatureParams(const pt_feature_params *params) {
    if(params != nullptr && (params->max_bounces < 0 || params->max_bounces > 32 || params->flags != 0)) {
        throw std::invalid_argument("ViewBatchRender::setFeatureParams: max_bounces must be 0..32 and flags 0");
    }
    if(frame_ != nullptr) {
        check(pt_frame_set_feature_params(frame_, params), "ViewBatchRender::setFeatureParams");
    }
}

void ViewBatchRender::setNoiseTarget(float target, float floor, float fraction) {
    if(!std::isfinite(target) || target < 0.0f || !std::isfinite(floor) || floor < 0.0f || !(fraction > 0.0f && fraction <= 1.0f)) {
        throw std::invalid_argument("ViewBatchRender::setNoiseTarget: target and floor must be finite and not negative, fraction in (0, 1]");
    }
    if(frame_ != nullptr) {
        check(pt_frame_set_noise_target(frame_, target, floor, fraction), "ViewBatchRender::setNoiseTarget");
    }
}

pt_frame_noise ViewBatchRender::noise() const {
    pt_frame_noise n{};
    if(frame_ != nullptr) {
        check(pt_frame_get_noise(frame_, &n, nullptr), "ViewBatchRender::noise");
    }
    return n;
}

std::vector<float> ViewBatchRender::errorMap() const {
    std::vector<float> map(static_cast<size_t>(width_) * static_cast<size_t>(height_) * seeds_.size(), -1.0f); // (a frame without pixels to render is finished)
    if(frame_ != nullptr) {
        pt_frame_noise n{};
        check(pt_frame_get_noise(frame_, &n, map.data()), "ViewBatchRender::errorMap");
    }
    return map;
}

bool ViewBatchRender::noiseTargetReached() const {
    return noise().target_reached != 0;
}

void ViewBatchRender::preview(std::vector<Image<>> &out, std::vector<std::int32_t> *samples, const pt_denoise_params *denoise) const {
    const size_t pixels = static_cast<size_t>(width_) * static_cast<size_t>(height_) * seeds_.size();
    if(samples != nullptr) {
        samples->assign(pixels, 0);
    }
    if(frame_ == nullptr) {
        out = split(stacked_);
        return;
    }
    std::vector<float> rgba(pixels * 4);
    check(pt_frame_preview(frame_, stacked_.data(), denoise, rgba.data(), samples != nullptr ? samples->data() : nullptr), "ViewBatchRender::preview");
    out = split(rgba);
}
