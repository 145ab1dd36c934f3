// src/host/temporal_denoise.cpp -- TemporalDenoiser and denoiseSequence of PathTrace/temporal_denoise.h on top of pt_render_features,
// pt_temporal_* and, with follow_motion, the scene's motion mark (include/pt_hip.h, include/pt_motion_shapes.h).
#include <PathTrace/temporal_denoise.h>

#include "../../include/pt_hip.h"
#include "job_params.h"

#include <cmath>
#include <stdexcept>
#include <vector>

using namespace pathtrace_host;

namespace {

    pt_temporal_params temporalParams(const TemporalDenoiseParams &p) {
        const DenoiseParams &s = p.spatial;
        if(s.iterations < 0 || s.iterations > 10) {
            throw std::invalid_argument("PathTrace: denoise iterations must be 0..10");
        }
        for(float sigma : {s.sigma_luminance, s.sigma_normal, s.sigma_depth, p.sigma_luminance_temporal, p.position_tolerance}) {
            if(!std::isfinite(sigma) || sigma < 0.0F) {
                throw std::invalid_argument("PathTrace: denoise sigmas and position_tolerance must be finite and not negative");
            }
        }
        for(float a : {p.alpha_color, p.alpha_moments}) {
            if(!(a > 0.0F && a <= 1.0F)) {
                throw std::invalid_argument("PathTrace: temporal alphas must be in (0, 1]");
            }
        }
        if(p.max_history < 1 || p.moments_min_history < 1 || !std::isfinite(p.normal_min)) {
            throw std::invalid_argument("PathTrace: max_history and moments_min_history must be >= 1, normal_min finite");
        }
        return pt_temporal_params{pt_denoise_params{s.iterations, s.sigma_luminance, s.sigma_normal, s.sigma_depth},
                                  p.alpha_color,
                                  p.alpha_moments,
                                  p.max_history,
                                  p.moments_min_history,
                                  p.sigma_luminance_temporal,
                                  p.normal_min,
                                  p.position_tolerance};
    }

} // namespace

TemporalDenoiser::TemporalDenoiser(const Scene &scene_, const RenderOptions &options_, const TemporalDenoiseParams &params) :
  scene(scene_), options(options_), follow_motion(params.follow_motion) {
    const pt_temporal_params p = temporalParams(params);
    if(options.image_width <= 0 || options.image_height <= 0) {
        throw std::invalid_argument("PathTrace: TemporalDenoiser needs a positive image size");
    }
    check(pt_temporal_create(sceneDevice(), options.image_width, options.image_height, &p, &handle), "TemporalDenoiser");
}

TemporalDenoiser::~TemporalDenoiser() {
    if(handle != nullptr) {
        pt_temporal_destroy(handle);
    }
}

Image<> TemporalDenoiser::push(const Image<> &frame, const Camera &camera) {
    if(frame.getWidth() != options.image_width || frame.getHeight() != options.image_height) {
        throw std::invalid_argument("PathTrace: TemporalDenoiser::push needs a frame of options.image_width x image_height");
    }
    const pt_camera_params cam = cameraParams(camera);
    const pt_options opt = renderOptions(options);
    pt_scene *replica = scene.deviceScenes().front();
    const size_t pixels = static_cast<size_t>(frame.getWidth()) * static_cast<size_t>(frame.getHeight());
    std::vector<float> features(pixels * 12);
    static_assert(sizeof(Color<float>) == 4 * sizeof(float), "Image<Color<float>> is a packed RGBA float array");
    Image<> out(frame.getWidth(), frame.getHeight());
    const size_t n_instances = follow_motion ? sceneInstanceCount(scene) : 0;
    if(n_instances > 0) {
        // The previous frame is the mark this object left on the scene at the end of its last push (include/pt_motion_shapes.h): the
        // instances' matrices and the meshes' shapes.  A scene that was only posed since takes pt_render_features_motion's own route
        // with the marked matrices; one whose meshes were deformed or morphed is reprojected per vertex.  A mark that is gone
        // (Scene::unmarkMotion) or a scene with another number of instances leaves no previous frame: the history is dropped.
        if(has_pose && (last_pose.size() != 16 * n_instances || pt_scene_get_motion_mark(replica, nullptr, nullptr) != PT_OK)) {
            reset();
        }
        std::vector<float> motion(pixels * 8);
        if(has_pose) {
            check(pt_render_features_motion_marked(replica, &cam, &opt, features.data(), motion.data()), "TemporalDenoiser::push (features and marked motion)");
        }
        else {
            check(pt_render_features_motion(replica, &cam, &opt, nullptr, features.data(), motion.data()), "TemporalDenoiser::push (features and motion)");
        }
        check(pt_temporal_denoise_motion(handle, reinterpret_cast<const float *>(frame.data()), features.data(), motion.data(), &cam,
                                         reinterpret_cast<float *>(out.data()), nullptr),
              "TemporalDenoiser::push");
        check(pt_scene_motion_mark(replica, nullptr), "TemporalDenoiser::push (mark)");
        last_pose.assign(16 * n_instances, 0.0F); // (its size is the instance count of the marked frame)
        has_pose = true;
        return out;
    }
    check(pt_render_features(replica, &cam, &opt, features.data()), "TemporalDenoiser::push (features)");
    check(pt_temporal_denoise(handle, reinterpret_cast<const float *>(frame.data()), features.data(), &cam, reinterpret_cast<float *>(out.data()), nullptr),
          "TemporalDenoiser::push");
    return out;
}

void TemporalDenoiser::reset() {
    check(pt_temporal_reset(handle), "TemporalDenoiser::reset");
    has_pose = false;
}

std::vector<Image<>> denoiseSequence(const std::vector<Image<>> &frames, const Scene &scene, const std::vector<const Camera *> &cameras, const RenderOptions &options,
                                     const TemporalDenoiseParams &params) {
    if(frames.size() != cameras.size()) {
        throw std::invalid_argument("PathTrace: denoiseSequence needs one camera per frame");
    }
    TemporalDenoiser denoiser(scene, options, params);
    std::vector<Image<>> out;
    out.reserve(frames.size());
    for(size_t v = 0; v < frames.size(); v++) {
        out.push_back(denoiser.push(frames[v], *cameras[v]));
    }
    return out;
}
