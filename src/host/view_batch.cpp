// src/host/view_batch.cpp -- processViews of PathTrace/view_batch.h on top of pt_render_views, and with allow_bias of
// pt_render_features_views and pt_denoise_views (include/pt_hip.h).
#include <PathTrace/denoise.h>
#include <PathTrace/view_batch.h>

#include "../../include/pt_hip.h"
#include "job_params.h"

#include <algorithm>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <vector>

using namespace pathtrace_host;

std::vector<Image<>> processViews(const Scene &scene, const std::vector<const Camera *> &cameras, const RenderOptions &options,
                                  const std::function<void(int, int)> &progress_callback, int worker_count, std::vector<std::uint64_t> *seeds) {
    if(cameras.empty()) {
        throw std::invalid_argument("PathTrace: processViews needs at least one camera");
    }
    std::vector<pt_camera_params> params;
    params.reserve(cameras.size());
    for(const Camera *camera : cameras) {
        if(camera == nullptr) {
            throw std::invalid_argument("PathTrace: processViews got a null camera");
        }
        params.push_back(cameraParams(*camera));
    }
    const std::vector<uint64_t> base_seeds = viewSeeds(cameras.size());
    if(seeds != nullptr) {
        *seeds = base_seeds;
    }
    const int width = std::max(options.image_width, 0);
    const int height = std::max(options.image_height, 0);
    std::vector<Image<>> views;
    views.reserve(cameras.size());
    for(size_t v = 0; v < cameras.size(); v++) {
        views.emplace_back(width, height);
    }
    if(width == 0 || height == 0) {
        return views;
    }
    // the library renders into one [V][H][W] array; the views are copied out of it
    static_assert(sizeof(Color<float>) == 4 * sizeof(float), "Image<Color<float>> is a packed RGBA float array");
    const size_t per_view = static_cast<size_t>(width) * static_cast<size_t>(height);
    std::vector<float> stacked(per_view * 4 * cameras.size());
    const pt_options opt = renderOptions(options);
    ForwardProgress forward{&progress_callback, nullptr};
    const std::vector<pt_scene *> &replicas = scene.deviceScenes();
    const int status = pt_render_views(replicas.data(), replicaCount(replicas, worker_count), params.data(), base_seeds.data(), static_cast<int32_t>(cameras.size()),
                                       &opt, stacked.data(), nullptr, &ForwardProgress::call, &forward);
    if(forward.failure) {
        std::rethrow_exception(forward.failure);
    }
    check(status, "processViews");
    if(options.allow_bias) {
        // as processJob denoises its frame, every view bit for bit, but with one launch per stage for the whole batch
        const DenoiseParams defaults;
        const pt_denoise_params p{defaults.iterations, defaults.sigma_luminance, defaults.sigma_normal, defaults.sigma_depth};
        std::vector<float> features(per_view * 12 * cameras.size());
        check(pt_render_features_views(replicas.front(), params.data(), static_cast<int32_t>(cameras.size()), &opt, features.data()), "processViews (features)");
        check(pt_denoise_views(sceneDevice(), stacked.data(), features.data(), width, height, static_cast<int32_t>(cameras.size()), &p, stacked.data()),
              "processViews (denoise)");
    }
    for(size_t v = 0; v < cameras.size(); v++) {
        std::memcpy(views[v].data(), stacked.data() + v * per_view * 4, per_view * 4 * sizeof(float));
    }
    return views;
}
