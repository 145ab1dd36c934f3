/* pt_motion.h -- motion-aware temporal denoising: where the surface a pixel sees was at the previous pose.  Part of the
 * C ABI of libpathtrace_hip.so: include/pt_hip.h includes this file behind pt_pose.h, which it needs; it is not meant to be included on
 * its own.
 *
 * pt_scene_pose moves the mesh instances of a scene between the frames of a sequence.  pt_temporal_denoise reprojects a pixel's CURRENT
 * position into the previous camera, which under a moved instance finds the history of another surface point (or none).  The entry points
 * here describe, per pixel, where the seen surface was at the previous pose, and reproject that point instead.
 *
 *   - pt_motion_table: pure host arithmetic, no device.  Per instance, with C = current[i] and P = previous[i] (fp32, rows):
 *       PT_MOTION_STATIC  P equals C bit for bit.  back = identity [I | 0], normal = identity.
 *       PT_MOTION_NONE    "no previous position": an entry of P or C that is not finite (a caller passes a NaN matrix for an instance that
 *                         was not there), a last row of either that is not (0, 0, 0, 1) by value, a 3x3 part of C or P whose double
 *                         determinant is 0 or not finite, or a rounded result that is not finite.  back = normal = 0.
 *       PT_MOTION_MOVED   everything else.  In double, A = C's 3x3 part, B = P's, inverses by adjugate / determinant, L = B A^-1:
 *                         back = [L | P_t - L C_t] (3 rows of 4: previous position = back * (current position, 1)),
 *                         normal = (A B^-1)^T (previous normal direction = normal * current normal), each rounded once to fp32.
 *     PT_ERR_INVALID for a null pointer with n > 0.
 *   - pt_render_features_motion[_device]: pt_render_features[_device] that also writes out_motion [height][width][2][4] from the same
 *     walks (nothing is traced twice); out_features is pt_render_features' result bit for bit.  previous_transforms: the matrices
 *     [n_instances][16] the instances had at the previous frame, or NULL = nothing moved (also for a scene without instances; with
 *     matrices such a scene is PT_ERR_UNSUPPORTED).  The current matrices are the scene's (pt_scene_get_pose).  Per feature ray that hits
 *     object o at pos with shading normal n: the instance whose non-empty object range holds o (objects of the description and spheres
 *     belong to none: static) gives
 *       static  pp = pos, pn = n, moved 0, none 0
 *       moved   pp[k] = ((back[k][0] pos.x + back[k][1] pos.y) + back[k][2] pos.z) + back[k][3];  v[k] likewise from normal[k] and n,
 *               without the last add;  pn = v * (1 / sqrtf((v.x v.x + v.y v.y) + v.z v.z)) if that sum is > 0, else 0;  moved 1, none 0
 *       none    pp = pn = 0, moved 1, none 1
 *     and a miss adds zeros.  Summed in ray order, then * 0.25f:
 *       out_motion[p][0] = (previous position xyz, fraction of rays on a moved surface)
 *       out_motion[p][1] = (previous normal xyz,   fraction of rays with no previous position)
 *     With every instance static, motion[0].xyz == features[2].xyz and motion[1].xyz == features[1].xyz bit for bit and both w are 0.
 *     Refusals: pt_render_features', and a null out_motion -- all before any device work.
 *   - pt_temporal_denoise_motion[_device]: pt_temporal_denoise[_device] with the frame's motion (NULL = those calls themselves).  For a
 *     covered pixel: motion[1].w > 0 -- no history (n = 1).  Otherwise Xr = motion[0].xyz / coverage and nr = motion[1].xyz at unit length
 *     take the place of the pixel's position and normal in the reprojection and in the taps' normal and position tests (the tolerance
 *     still comes from the current hit distance).  The pixel is its own tap only if the camera equals the previous one bit for bit AND
 *     motion[0].w == 0; otherwise Xr is projected into the previous camera.  What the push stores for the next one stays the current
 *     position and normal; blend, variance, a-trous passes and finish are unchanged.  A motion in which every instance is static gives
 *     pt_temporal_denoise's result bit for bit.
 *
 * Left out: view batches (there is no pt_render_features_motion_views) and followed features (motion describes the FIRST hit; the
 * followed features' virtual positions have no previous pose), motion blur.  Meshes that change shape between two frames are described
 * by pt_motion_shapes.h, not here: these entry points know an instance by its matrix alone. */
#ifndef PT_MOTION_ABI_H
#define PT_MOTION_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

enum { PT_MOTION_STATIC = 0, PT_MOTION_MOVED = 1, PT_MOTION_NONE = 2 };

typedef struct pt_temporal pt_temporal;

int pt_motion_table(const float *current /* [n][16], rows */, const float *previous /* [n][16] */, uint32_t n, uint8_t *out_kind /* [n] */,
                    float *out_back /* [n][12] */, float *out_normal /* [n][9] */);
int pt_render_features_motion(pt_scene *scene, const pt_camera_params *camera, const pt_options *options,
                              const float *previous_transforms /* [n_instances][16] or NULL */, float *out_features /* [H][W][3][4] */,
                              float *out_motion /* [H][W][2][4] */);
int pt_render_features_motion_device(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const float *previous_transforms,
                                     float *d_out_features, float *d_out_motion, void *stream);
int pt_temporal_denoise_motion(pt_temporal *t, const float *rgba, const float *features, const float *motion /* may be NULL */,
                               const pt_camera_params *camera, float *out_rgba, int32_t *out_history);
int pt_temporal_denoise_motion_device(pt_temporal *t, const float *d_rgba, const float *d_features, const float *d_motion /* may be NULL */,
                                      const pt_camera_params *camera, float *d_out_rgba, int32_t *d_out_history, void *stream);

#ifdef __cplusplus
}
#endif

#endif
