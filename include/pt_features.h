/* pt_features.h -- denoiser features that follow mirrors and glass to the first diffuse hit.  Part of the C ABI of
 * libpathtrace_hip.so: include/pt_hip.h includes this file, which is not meant to be included on its own.
 *
 * The first-hit features of pt_render_features describe, on a mirror or a glass surface, that surface itself -- a smooth normal, a smooth t,
 * a white specular albedo -- and leave only the filter's luminance term between it and whatever is seen in the mirror or through the glass.
 * A FOLLOWED feature ray goes on instead.  The rays are pt_render_features' own: 4 deterministic primary rays per pixel, aperture ignored,
 * no jitter.  Every ray carries a tint T = (1, 1, 1), a length L = 0, a bounce count b = 0 and its primary origin and direction o0, d0,
 * and repeats:
 *   - closest hit.  A miss, at any bounce, ends the ray: it adds zeros and no coverage, exactly as a first-hit miss does.
 *   - a hit at distance t:  L = L + t (fp32, in segment order);  pos = o + d * t;  n = the object's shading normal;  the material.
 *   - TERMINAL if the material is Lambertian, or there is none, or b == max_bounces.  The ray contributes
 *         albedo    T * (diffuse for Lambertian, specular for glass or mirror, white without a material), coverage 1
 *         normal    this hit's n;  t = L, the summed length of the segments
 *         position  o0 + d0 * L: the unfolded ("virtual") position -- for a plane mirror the mirror image of the hit point
 *         emission  T * the material's emission
 *   - a mirror: the next ray is the one BSDF::propagateRay returns (it draws nothing), the pass-through of a one-way mirror included.
 *   - glass: a deterministic branch, no draw.  Where sin_theta_t >= 1 (the reference's Bernoulli has p = 1 there: total internal reflection)
 *     the reflection branch, everywhere else the REFRACTION branch, each with propagateRay's arithmetic operation for operation, the
 *     pos + dir * epsilon origin included.  (The likelier Fresnel branch is not followed: the branch is a function of the geometry alone.)
 *   - T = T * rgb of BSDF::getSpectrum(d, next d, n, white) -- what a path's bounce multiplies its spectrum by -- then b += 1, and on.
 * A ray makes at most max_bounces + 1 walks: that count bounds the work, never the geometry.  A NaN direction misses and ends as a miss.
 *
 * out_features has pt_render_features' layout and order: [height][width][3][4] floats, the 4 rays summed in ray order, then * 0.25f; [2].w is
 * the luminance of the mean tinted emission.  max_bounces = 0 gives pt_render_features' result bit for bit.
 *
 * `options`: image_width, image_height AND epsilon are read (pt_render_features reads only the sizes): epsilon is the offset of every
 * continued ray's origin, as in a render.
 *
 * What the filters make of them.  The depth term compares t = L along the unfolded ray, so an edge seen in a mirror is an edge; normals are
 * those of the surfaces seen, not the mirror's.  pt_temporal_denoise takes its features from the caller, so followed ones may be passed
 * there: it reprojects the virtual position, which is exact for plane mirrors and an approximation behind curved mirrors and glass
 * (the C++ TemporalDenoiser / denoiseSequence compute first-hit features themselves and keep doing so).
 *
 *   - pt_render_features_followed[_views][_device]: the followed forms of pt_render_features[_views][_device], same buffers, same stream
 *     rules; view v of a views result is bit for bit the single-frame result for cameras[v].  params NULL = pt_feature_params_default.
 *     PT_ERR_INVALID before anything is uploaded or launched: a null scene, camera, options or output, a size <= 0, n_views <= 0, more than
 *     0x0fffffff pixels, max_bounces outside 0..32, flags != 0, an epsilon that is negative or not finite.
 *   - pt_frame_set_feature_params: the denoised previews of `frame` (pt_frame_preview, pt_frame_preview_measured; single and view frames)
 *     use followed features with these parameters and the frame's own epsilon from then on; NULL restores the first-hit features, which
 *     is how a frame starts.  The features a preview has cached are dropped: the next denoised preview computes them again.  Changes
 *     nothing the frame renders.  PT_ERR_INVALID for a null frame, or parameters (or a frame epsilon) the render entries refuse.
 * Every other entry point keeps first-hit features, and its results bit for bit. */
#ifndef PT_FEATURES_H
#define PT_FEATURES_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_feature_params {
    int32_t max_bounces; /* 0..32, default 8 */
    int32_t flags;       /* must be 0 */
} pt_feature_params;
int pt_feature_params_default(pt_feature_params *out);
int pt_render_features_followed(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const pt_feature_params *params, float *out_features);
int pt_render_features_followed_device(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const pt_feature_params *params,
                                       float *d_out_features, void *stream);
int pt_render_features_followed_views(pt_scene *scene, const pt_camera_params *cameras, int32_t n_views, const pt_options *options,
                                      const pt_feature_params *params, float *out_features);
int pt_render_features_followed_views_device(pt_scene *scene, const pt_camera_params *cameras, int32_t n_views, const pt_options *options,
                                             const pt_feature_params *params, float *d_out_features, void *stream);
int pt_frame_set_feature_params(pt_frame *frame, const pt_feature_params *params /* NULL = first-hit features */);

#ifdef __cplusplus
}
#endif

#endif
