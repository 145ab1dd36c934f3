/* pt_gather.h -- how much light arrives at surface points: occlusion, direct light, full paths.
 * Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h includes this file at its end; it is not meant to be included on its own.
 *
 * A point is a position P and a unit normal N (six floats).  It stands for a receiver with the default handler (PT_NO_MATERIAL): white
 * Lambertian, no emission.  A call takes `samples` samples at every point and returns one 32-byte pt_gather_result per point.
 *
 * The sample.  Sample s of point i -- i is the point's index in the call -- has an engine of its own, RandomEngine(pt_pixel_seed(base_seed,
 * x = s, y = i)).  A value depends on nothing else: not on the other points, and not on how the call is cut into launches.
 *
 *   PT_GATHER_OCCLUSION  next = LambertianBRDF::propagateRay(ray with dir -N, P, N, epsilon, re); the sample is occluded iff the closest
 *                        hit of `next` has 0 <= t < distance (pt_occluded_rays' definition and its walk; distance = +inf is allowed).
 *                        occluded = the number of occluded samples; value[0..2] = (float)(samples - occluded) / (float)samples.
 *   PT_GATHER_DIRECT     lines 74-103 of the reference's worker.cpp once, with pos = P, n = N, ray.dir = -N, sample_spectrum = 1,
 *                        sample_divisor = sample_bounce_pd = 1.0 (double, as there).  No roulette number is drawn.  The sample is
 *                        out_spectrum.
 *   PT_GATHER_PATHS      getSample's loop entered at line 55 with a virtual first vertex: pos = P, n = N, ray.dir = -N, the default
 *                        material and BSDF, path_length = 1, every accumulator at its initial value; from there unchanged: emission
 *                        (zero at the virtual vertex), the roulette draw, the lights, the bounce, and every later real vertex exactly
 *                        as the path kernel shades it.  The sample is out_spectrum.
 *   DIRECT and PATHS: value[c] = (...((0 + s_0[c]) + s_1[c]) + ...) / (float)samples in fp32, in sample order; occluded = 0.
 *   value[3] = 1 and samples = the samples taken, for every kind.
 *
 * Entry points.  The host forms take host memory and return when the results are there.  The _device forms take DEVICE pointers for
 * points and results and a hipStream_t, ordered as pt_query_rays_device orders its work; a null stream makes the call wait.
 *   - pt_gather_points: n points.
 *   - pt_gather_frame: the first hit of the ray through each pixel centre (the ray of pt_query_frame: no aperture, no jitter), the shading
 *     normal negated where dot(normal, d) > 0; out[y * image_width + x].  A pixel whose ray hits nothing gets an all-zero record, samples =
 *     0.  Point i is pixel i.
 *   - pt_gather_instance: the three corners of every surviving triangle of a mesh instance with the corner normals -- the out_pos and
 *     out_nrm of pt_scene_get_triangles for the instance's range (pt_scene_instance_ranges) --, out[triangle][corner]; point i is corner
 *     i % 3 of triangle i / 3.  The points are made on the device; no triangle is copied to the host.  PT_ERR_UNSUPPORTED for a scene
 *     without mesh instances.
 * The work is cut into launches of whole points with at most PT_GATHER_CHUNK (an environment variable read per call; default 4194304)
 * (point, sample) pairs each -- one point where a point alone has more --, over a workspace that belongs to the scene.
 *
 * Refusals, all before any device work, PT_ERR_INVALID: a null argument (n == 0 needs no arrays and launches nothing), an unknown kind,
 * samples < 1, points x samples above 0x7fffffff, an epsilon that is negative or NaN, for OCCLUSION a distance that is not greater than 0
 * (NaN included), an instance out of range, an image size that is not positive.  Every call holds the scene's render lock, changes nothing in
 * the scene, and is allowed with a live pt_frame and with or without a motion mark.
 *
 * Left out: materials other than the white receiver, an inset of corner points, more than one device, view batches, a bound on the path
 * length (the reference has none). */
#ifndef PT_GATHER_ABI_H
#define PT_GATHER_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

#define PT_GATHER_OCCLUSION 0
#define PT_GATHER_DIRECT    1
#define PT_GATHER_PATHS     2

typedef struct pt_gather_params { int32_t kind; int32_t samples; float epsilon; float distance; uint64_t base_seed; } pt_gather_params;
typedef struct pt_gather_result { float value[4]; uint32_t samples; uint32_t occluded; uint32_t pad[2]; } pt_gather_result; /* 32 bytes */

/* kind PT_GATHER_OCCLUSION, 16 samples, epsilon 1e-3, distance +inf, base_seed 0 */
int pt_gather_params_default(pt_gather_params *out);
int pt_gather_points(pt_scene *scene, const float *points /* [n][6]: position, normal */, size_t n, const pt_gather_params *params, pt_gather_result *out /* [n] */);
int pt_gather_points_device(pt_scene *scene, const float *d_points, size_t n, const pt_gather_params *params, pt_gather_result *d_out, void *stream);
int pt_gather_frame(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const pt_gather_params *params, pt_gather_result *out /* [H][W] */);
int pt_gather_frame_device(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const pt_gather_params *params, pt_gather_result *d_out, void *stream);
int pt_gather_instance(pt_scene *scene, uint32_t instance, const pt_gather_params *params, pt_gather_result *out /* [n_objects of the instance][3] */);

#ifdef __cplusplus
}
#endif

#endif
