/* pt_radiance.h -- the radiance that arrives along rays the caller chooses, and captures: whole images of such rays made on the device by
 * one of four camera models -- equirectangular panorama, cube map, equidistant fisheye, orthographic.
 * Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h includes this file behind pt_gather.h; it is not meant to be included on its own.
 *
 * A call takes `samples` samples of every ray, or of every pixel of a capture, and returns one 32-byte pt_radiance_result each: the mean
 * radiance with its alpha, and three counts.  A capture's results are in row order, [height][width].
 *
 * The sample.  Sample s of ray or pixel i has an engine of its own, RandomEngine(pt_pixel_seed(base_seed, x = s, y = i)) (pt_gather.h's
 * rule); i is the ray's index in the call, or py * width + px for a pixel.  A value depends on nothing else: not on the other rays, and not
 * on how the call is cut into launches.
 *   pt_radiance_rays: the sample's ray is (o, d) as given; d is not normalised, as pt_intersect_batch takes it.  No number is drawn before
 *   the loop.  L_s is getSample's result behind that ray -- the reference's loop entered at worker.cpp:44 with path_length = 0 and every
 *   accumulator at its initial value, every vertex shaded as the path kernel shades it --, and its alpha is getSample's: 1 where the first
 *   walk hits, 0 where it misses.
 *
 * The pixel sample of a capture, in fp32, in this order.  With `jitter`, u1 = dist(re); u2 = dist(re) are drawn in that order; otherwise
 * u1 = u2 = 0.5f and nothing is drawn.  sx = ((float)px + u1) / (float)width;  sy = ((float)py + u2) / (float)height  (CUBE uses the
 * face-local forms below instead).  a = 2.0f * sx - 1.0f;  b = 1.0f - 2.0f * sy.  A local direction l = (lx, ly, lz) becomes
 * d[k] = ((right[k] * lx) + (up[k] * ly)) + (forward[k] * lz); the basis is used as given, never normalised, never re-orthogonalised.
 *   EQUIRECT  phi = (2.0f * PT_PI_F) * (sx - 0.5f);  theta = PT_PI_F * sy;  sincosf of both (glibc's, restated on the device, as the
 *             light-probe sampler calls it);  l = (st * sp, ct, st * cp);  d is used as it is.  Row 0 looks along `up`, the image centre
 *             along `forward`.
 *   CUBE      width == 6 * height;  N = height;  face k = px / N;  a = 2.0f * (((float)(px - k * N) + u1) / (float)N) - 1.0f;
 *             b = 1.0f - 2.0f * (((float)py + u2) / (float)N);  l is, for face 0: (1, b, -a), 1: (-1, b, a), 2: (a, 1, -b), 3: (a, -1, b),
 *             4: (a, b, 1), 5: (-a, b, -1) -- on each face a grows to the viewer's right and b upwards;  d is normalised as the reference's
 *             vec3::normalize does it (inv = 1.0f / sqrtf(dot); d * inv).
 *   FISHEYE   equidistant;  width == height;  rr = sqrtf(a * a + b * b);  if rr > 1.0f the sample has no ray (`outside` below);
 *             theta = rr * (0.5f * fov);  sincosf;  l = (0, 0, 1) if rr == 0.0f, else ((st * a) / rr, (st * b) / rr, ct);  d is used as it
 *             is.  fov is the full angle across the image circle in radians, 0 < fov <= 2 pi.
 *   ORTHO     o[k] = (origin[k] + right[k] * (a * extent[0])) + up[k] * (b * extent[1]);  d = forward as given.  extent holds half the
 *             width and half the height of the window in scene units.
 * Every model but ORTHO starts at `origin`.
 *
 * The record.  term_s = L_s (rgba) for a traced sample.  For j in 0..63, partial_j = the fp32 sum from +0 of term_s over s = j, j + 64,
 * j + 128, ... in increasing s (+0 where there is no such s).  sum = (...((0 + partial_0) + partial_1) + ... + partial_63).
 * value = sum / (float)samples.  The strided order is pt_light_probes.h's and part of the definition: one wavefront reduces one ray or
 * pixel with coalesced loads, whatever the chunking.  With samples == 1, value is L_0, bit for bit.
 *   samples   the samples taken
 *   missed    the samples whose first walk hits nothing
 *   outside   the samples with no ray (FISHEYE, rr > 1): such a sample contributes (0, 0, 0, 0) and draws nothing after its jitter; it is
 *             counted in `samples` and not in `missed`, so the circle's edge is antialiased by the mean
 *
 * Entry points.  The host forms take host memory and return when the results are there.  The _device forms take DEVICE pointers for the
 * rays and the results, and a hipStream_t, ordered as pt_gather_points_device orders its work; a null stream makes the call wait.  The
 * work is cut into launches of whole rays or pixels with at most PT_RADIANCE_CHUNK (an environment variable read per call; default
 * 2097152) (ray or pixel, sample) pairs each -- one ray or pixel where it alone has more --, over a workspace that is kept per device.
 * The contents of `rays` are not inspected, as pt_query_rays does not inspect its rays.
 *
 * Refusals, all before any device work and before the scene is locked, PT_ERR_INVALID: a null argument (n == 0 needs no arrays and
 * launches nothing), samples < 1, rays x samples or pixels x samples above 0x7fffffff, an epsilon that is negative or NaN, an unknown
 * model, a width or height below 1, a jitter other than 0 or 1, CUBE with width != 6 * height, FISHEYE with width != height or with a fov
 * that is NaN, <= 0 or > 2 pi, ORTHO with an extent that is not finite or not > 0, any of the twelve floats of origin and basis not
 * finite.  Every call holds the scene's render lock, changes nothing in the scene, and is allowed with a live pt_frame and with or without
 * a motion mark.
 *
 * Left out: adaptive sampling and the per-pixel estimator, resumable, progressive and checkpointed captures, denoiser features for
 * captures, non-square fisheye, thin-lens apertures on captures, more than one device, view batches. */
#ifndef PT_RADIANCE_ABI_H
#define PT_RADIANCE_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

#define PT_CAPTURE_EQUIRECT 0
#define PT_CAPTURE_CUBE     1
#define PT_CAPTURE_FISHEYE  2
#define PT_CAPTURE_ORTHO    3

typedef struct pt_radiance_params { int32_t samples; float epsilon; uint64_t base_seed; } pt_radiance_params; /* 16 bytes */
typedef struct pt_radiance_result { float value[4]; uint32_t samples, missed, outside; uint32_t pad; } pt_radiance_result; /* 32 bytes */
typedef struct pt_capture_desc {
    int32_t model, width, height, jitter;         /* jitter: 0 = pixel centres, 1 = a jittered position per sample */
    float origin[3], right[3], up[3], forward[3]; /* used as given: never normalised, never re-orthogonalised */
    float fov;                                    /* FISHEYE: the full angle across the image circle, radians, 0 < fov <= 2 pi */
    float extent[2];                              /* ORTHO: half width and half height of the window, scene units */
    uint32_t pad;
} pt_capture_desc; /* 80 bytes */

/* 64 samples, epsilon 1e-3, base_seed 0 */
int pt_radiance_params_default(pt_radiance_params *out);
int pt_radiance_rays(pt_scene *scene, const float *rays /* [n][6]: origin, direction */, size_t n, const pt_radiance_params *params, pt_radiance_result *out /* [n] */);
int pt_radiance_rays_device(pt_scene *scene, const float *d_rays, size_t n, const pt_radiance_params *params, pt_radiance_result *d_out, void *stream);
int pt_radiance_capture(pt_scene *scene, const pt_capture_desc *capture, const pt_radiance_params *params, pt_radiance_result *out /* [height][width] */);
int pt_radiance_capture_device(pt_scene *scene, const pt_capture_desc *capture, const pt_radiance_params *params, pt_radiance_result *d_out, void *stream);

#ifdef __cplusplus
}
#endif

/* The same samples split by emitter group and bounce depth, and the mix of such passes (pt_light_passes_rays, pt_light_passes_capture,
 * pt_light_passes_mix): they take this file's parameters, capture and record, and are declared, with their contracts, in: */
#include "pt_light_passes.h"

#endif
