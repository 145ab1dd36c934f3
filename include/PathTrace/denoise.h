// PathTrace/denoise.h -- feature-guided denoising of a finished frame (an extension of PathTrace/worker.h).
#ifndef PATHTRACE_DENOISE_H
#define PATHTRACE_DENOISE_H

#include <PathTrace/camera.h>
#include <PathTrace/image/image.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

// The filter's parameters (pt_denoise_params of pt_hip.h); the defaults are SVGF's, but for sigma_luminance.  A sigma of 0 turns its term off.
struct DenoiseParams {
    int iterations = 5;            // a-trous passes, 0..10
    float sigma_luminance = 32.0F; // luminance edge-stopping, in standard deviations of the local luminance
    float sigma_normal = 128.0F;   // exponent of max(0, n_p . n_q)
    float sigma_depth = 1.0F;      // depth edge-stopping, in units of the depth change the local gradient predicts
};

// What processJob returns when options.allow_bias is set, for callers who keep the noisy frame as well: the first-hit features of
// camera's view of scene (4 deterministic primary rays per pixel, the aperture ignored) guide an edge-avoiding a-trous filter -- the
// spatial part of SVGF -- over `frame`.  Computed on the scene's first device replica.  frame must be options.image_width x image_height;
// alpha is copied.  denoise(processJob(job without bias), scene, camera, options) equals processJob(job with bias) bit for bit when
// both renders have the same seed ($PATHTRACE_SEED).  Throws std::invalid_argument for a frame of another size or parameters outside
// their range, std::runtime_error if the device fails.
Image<> denoise(const Image<> &frame, const Scene &scene, const Camera &camera, const RenderOptions &options, const DenoiseParams &params = {});

// Features that follow mirrors and glass to the first diffuse hit (pt_feature_params of pt_features.h): a feature ray
// that hits a mirror or glass goes on -- deterministically: a mirror's reflection, glass's refraction, or its reflection where that is
// total -- for at most max_bounces bounces, and describes what is seen in the mirror or through the glass.
struct FeatureParams {
    int max_bounces = 8; // 0..32; 0 gives the first-hit features
};

// denoise with followed features: the same filter, guided by what the mirrors and the glass show.  options.epsilon is read as well (the
// offset of a continued ray's origin).  processJob / processViews with allow_bias keep the first-hit features.  Throws as denoise does,
// and std::invalid_argument for max_bounces outside 0..32 or an epsilon that is negative or not finite.
Image<> denoise(const Image<> &frame, const Scene &scene, const Camera &camera, const RenderOptions &options, const DenoiseParams &params,
                const FeatureParams &features);

#endif
