// src/host/denoise.cpp -- denoise of PathTrace/denoise.h (and the allow_bias step of processJob / processViews) on top of
// pt_render_features[_followed] and pt_denoise (include/pt_hip.h).
#include <PathTrace/denoise.h>

#include "../../include/pt_hip.h"
#include "job_params.h"

#include <cmath>
#include <stdexcept>
#include <vector>

using namespace pathtrace_host;

namespace {

// follow == nullptr: the first-hit features of pt_render_features; else the followed ones of pt_render_features_followed
Image<> denoiseWith(const Image<> &frame, const Scene &scene, const Camera &camera, const RenderOptions &options, const DenoiseParams &params,
                    const pt_feature_params *follow) {
    if(frame.getWidth() != options.image_width || frame.getHeight() != options.image_height) {
        throw std::invalid_argument("PathTrace: denoise needs a frame of options.image_width x options.image_height");
    }
    if(params.iterations < 0 || params.iterations > 10) {
        throw std::invalid_argument("PathTrace: denoise iterations must be 0..10");
    }
    for(float sigma : {params.sigma_luminance, params.sigma_normal, params.sigma_depth}) {
        if(!std::isfinite(sigma) || sigma < 0.0F) {
            throw std::invalid_argument("PathTrace: denoise sigmas must be finite and not negative");
        }
    }
    Image<> out(frame.getWidth(), frame.getHeight());
    if(frame.getWidth() <= 0 || frame.getHeight() <= 0) {
        return out;
    }
    const pt_camera_params cam = cameraParams(camera);
    const pt_options opt = renderOptions(options);
    pt_scene *replica = scene.deviceScenes().front();
    std::vector<float> features(static_cast<size_t>(frame.getWidth()) * static_cast<size_t>(frame.getHeight()) * 12);
    if(follow != nullptr) {
        check(pt_render_features_followed(replica, &cam, &opt, follow, features.data()), "denoise (followed features)");
    }
    else {
        check(pt_render_features(replica, &cam, &opt, features.data()), "denoise (features)");
    }
    static_assert(sizeof(Color<float>) == 4 * sizeof(float), "Image<Color<float>> is a packed RGBA float array");
    const pt_denoise_params p{params.iterations, params.sigma_luminance, params.sigma_normal, params.sigma_depth};
    check(pt_denoise(sceneDevice(), reinterpret_cast<const float *>(frame.data()), features.data(), frame.getWidth(), frame.getHeight(), &p,
                     reinterpret_cast<float *>(out.data())),
          "denoise");
    return out;
}

} // namespace

Image<> denoise(const Image<> &frame, const Scene &scene, const Camera &camera, const RenderOptions &options, const DenoiseParams &params) {
    return denoiseWith(frame, scene, camera, options, params, nullptr);
}

Image<> denoise(const Image<> &frame, const Scene &scene, const Camera &camera, const RenderOptions &options, const DenoiseParams &params,
                const FeatureParams &features) {
    if(features.max_bounces < 0 || features.max_bounces > 32) {
        throw std::invalid_argument("PathTrace: FeatureParams::max_bounces must be 0..32");
    }
    if(!std::isfinite(options.epsilon) || options.epsilon < 0.0F) {
        throw std::invalid_argument("PathTrace: followed features need a finite, non-negative RenderOptions::epsilon");
    }
    const pt_feature_params follow{features.max_bounces, 0};
    return denoiseWith(frame, scene, camera, options, params, &follow);
}
