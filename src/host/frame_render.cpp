// src/host/frame_render.cpp -- FrameRender of PathTrace/frame_render.h on top of the resumable frames of the C ABI (pt_frame_*).
#include <PathTrace/frame_render.h>

#include "../../include/pt_hip.h"
#include "job_params.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <vector>

using namespace pathtrace_host;

FrameRender::FrameRender(const FrameRenderJob &job, int worker_count) :
  image_(std::max(job.options.image_width, 0), std::max(job.options.image_height, 0)) {
    seed_ = jobSeed();
    if(image_.getWidth() == 0 || image_.getHeight() == 0) {
        complete_ = true;
        return;
    }
    const pt_camera_params camera = cameraParams(job.camera);
    const pt_options options = renderOptions(job.options);
    tiles_ = jobTiles(static_cast<int>(image_.getWidth()), static_cast<int>(image_.getHeight()));
    const std::vector<pt_scene *> &replicas = job.scene.deviceScenes();
    check(pt_frame_create(replicas.data(), replicaCount(replicas, worker_count), &camera, &options, tiles_.data(), tiles_.size(), seed_, &frame_), "FrameRender");
}

// FrameRender::load
FrameRender::FrameRender(const Scene &scene, const std::vector<std::uint8_t> &blob, int worker_count) : image_(0, 0) {
    pt_checkpoint_info info{};
    check(pt_checkpoint_inspect(blob.data(), blob.size(), &info), "FrameRender::load");
    if(info.n_views != 1) {
        throw std::runtime_error("PathTrace: FrameRender::load: the checkpoint is of a view batch (ViewBatchRender::load takes it)");
    }
    pt_checkpoint_header header;
    std::memcpy(&header, blob.data(), sizeof(header));
    seed_ = header.base_seed;
    image_ = Image<>(static_cast<size_t>(info.options.image_width), static_cast<size_t>(info.options.image_height));
    tiles_.resize(static_cast<size_t>(info.n_tiles));
    if(!tiles_.empty()) {
        std::memcpy(tiles_.data(), blob.data() + (sizeof(header) + info.bytes_tables + 15) / 16 * 16, tiles_.size() * sizeof(pt_tile));
    }
    const std::vector<pt_scene *> &replicas = scene.deviceScenes();
    check(pt_frame_checkpoint_load(replicas.data(), replicaCount(replicas, worker_count), blob.data(), blob.size(), reinterpret_cast<float *>(image_.data()), &frame_),
          "FrameRender::load");
    complete_ = info.streams_finished == info.n_streams;
}

void FrameRender::save(std::vector<std::uint8_t> &blob) const {
    blob.clear();
    if(frame_ == nullptr) {
        return; // (a frame without pixels has nothing to save)
    }
    size_t bytes = 0;
    check(pt_frame_checkpoint_size(frame_, &bytes), "FrameRender::save");
    blob.resize(bytes);
    check(pt_frame_checkpoint_save(frame_, reinterpret_cast<const float *>(image_.data()), blob.data(), blob.size(), &bytes), "FrameRender::save");
    blob.resize(bytes);
}

FrameRender::~FrameRender() {
    if(frame_ != nullptr) {
        pt_frame_destroy(frame_);
    }
}

bool FrameRender::render(RenderControl &control, const std::function<void(int, int)> &progress_callback) {
    control.cancelled_ = false;
    control.finished_.clear();
    control.tile_count_ = tiles_.size();
    if(frame_ == nullptr) {
        return complete_;
    }
    static_assert(sizeof(Color<float>) == 4 * sizeof(float), "Image<Color<float>> is a packed RGBA float array");
    ForwardProgress forward{&progress_callback, nullptr};
    std::vector<uint8_t> done(tiles_.size(), 0);
    control.ctl_.tile_done = done.data();
    const int status = pt_frame_render(frame_, reinterpret_cast<float *>(image_.data()), nullptr, &ForwardProgress::call, &forward, &control.ctl_);
    control.ctl_.tile_done = nullptr;
    if(forward.failure) {
        std::rethrow_exception(forward.failure);
    }
    if(status != PT_ERR_CANCELLED) {
        check(status, "FrameRender::render");
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

pt_frame_info FrameRender::info() const {
    pt_frame_info i{};
    if(frame_ != nullptr) {
        check(pt_frame_get_info(frame_, &i), "FrameRender::info");
    }
    return i;
}

void FrameRender::setProgressive(int quantum, int max_passes_per_call) {
    if(quantum < 0) {
        throw std::invalid_argument("FrameRender::setProgressive: negative quantum");
    }
    if(frame_ != nullptr) {
        check(pt_frame_set_progressive(frame_, quantum, max_passes_per_call), "FrameRender::setProgressive");
    }
}

pt_frame_progress FrameRender::progress() const {
    pt_frame_progress p{};
    if(frame_ != nullptr) {
        check(pt_frame_get_progress(frame_, &p), "FrameRender::progress");
    }
    return p;
}

void FrameRender::setFeatureParams(const pt_feature_params *params) {
    if(params != nullptr && (params->max_bounces < 0 || params->max_bounces > 32 || params->flags != 0)) {
        throw std::invalid_argument("FrameRender::setFeatureParams: max_bounces must be 0..32 and flags 0");
    }
    if(frame_ != nullptr) {
        check(pt_frame_set_feature_params(frame_, params), "FrameRender::setFeatureParams");
    }
}

void FrameRender::setNoiseTarget(float target, float floor, float fraction) {
    if(!std::isfinite(target) || target < 0.0f || !std::isfinite(floor) || floor < 0.0f || !(fraction > 0.0f && fraction <= 1.0f)) {
        throw std::invalid_argument("FrameRender::setNoiseTarget: target and floor must be finite and not negative, fraction in (0, 1]");
    }
    if(frame_ != nullptr) {
        check(pt_frame_set_noise_target(frame_, target, floor, fraction), "FrameRender::setNoiseTarget");
    }
}

pt_frame_noise FrameRender::noise() const {
    pt_frame_noise n{};
    if(frame_ != nullptr) {
        check(pt_frame_get_noise(frame_, &n, nullptr), "FrameRender::noise");
    }
    return n;
}

std::vector<float> FrameRender::errorMap() const {
    std::vector<float> map(static_cast<size_t>(image_.getWidth()) * static_cast<size_t>(image_.getHeight()), -1.0f); // (a frame without pixels to render is finished)
    if(frame_ != nullptr) {
        pt_frame_noise n{};
        check(pt_frame_get_noise(frame_, &n, map.data()), "FrameRender::errorMap");
    }
    return map;
}

bool FrameRender::noiseTargetReached() const {
    return noise().target_reached != 0;
}

void FrameRender::preview(Image<> &out, std::vector<std::int32_t> *samples, const pt_denoise_params *denoise) const {
    if(out.getWidth() != image_.getWidth() || out.getHeight() != image_.getHeight()) {
        out = Image<>(image_.getWidth(), image_.getHeight());
    }
    if(samples != nullptr) {
        samples->assign(static_cast<size_t>(image_.getWidth()) * static_cast<size_t>(image_.getHeight()), 0);
    }
    if(frame_ == nullptr) {
        return;
    }
    check(pt_frame_preview(frame_, reinterpret_cast<const float *>(image_.data()), denoise, reinterpret_cast<float *>(out.data()),
                           samples != nullptr ? samples->data() : nullptr),
          "FrameRender::preview");
}

std::vector<float> FrameRender::variance() const {
    std::vector<float> map(4 * static_cast<size_t>(image_.getWidth()) * static_cast<size_t>(image_.getHeight()), 0.0f);
    if(frame_ != nullptr) {
        check(pt_frame_get_variance(frame_, map.data()), "FrameRender::variance");
    }
    return map;
}

void FrameRender::previewMeasured(Image<> &out, std::vector<std::int32_t> *samples, const pt_denoise_measured_params *params) const {
    if(out.getWidth() != image_.getWidth() || out.getHeight() != image_.getHeight()) {
        out = Image<>(image_.getWidth(), image_.getHeight());
    }
    if(samples != nullptr) {
        samples->assign(static_cast<size_t>(image_.getWidth()) * static_cast<size_t>(image_.getHeight()), 0);
    }
    if(frame_ == nullptr) {
        return;
    }
    check(pt_frame_preview_measured(frame_, reinterpret_cast<const float *>(image_.data()), params, reinterpret_cast<float *>(out.data()),
                                    samples != nullptr ? samples->data() : nullptr),
          "FrameRender::previewMeasured");
}
