/* pt_light_probes.h -- light probes: the radiance that arrives at free points from every direction, projected onto spherical harmonics;
 * grids of such probes; and the lookup that turns a grid into light at a point with a normal.
 * Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h includes this file at its end; it is not meant to be included on its own.
 *
 * A light probe is a position P of three floats.  It has no normal.  A call takes `samples` samples at every probe and returns one
 * 128-byte pt_light_probe per probe: 9 SH coefficients (bands 0..2) per colour channel, and three counts.
 *
 * The sample.  Sample s of probe i -- i is the probe's index in the call -- has an engine of its own, RandomEngine(pt_pixel_seed(base_seed,
 * x = s, y = i)) (pt_gather.h's rule).  A value depends on nothing else: not on the other probes, and not on how the call is cut into
 * launches.  The direction is uniform on the sphere, formed in fp32 in this order:
 *   u1 = dist(re); u2 = dist(re); z = 1.0f - 2.0f * u1; r = sqrtf(1.0f - z * z); phi = 2.0f * PT_PI_F * u2 (LambertianBRDF's association);
 *   sincosf(phi, &sn, &cs); d = (r * cs, r * sn, z), used as it is and not normalised.
 * The sample's radiance L_s is getSample's out_spectrum behind the ray (P, d): the reference's loop entered at worker.cpp:44 with
 * path_length = 0 and every accumulator at its initial value, every vertex shaded as the path kernel shades it.
 *   samples     the samples taken
 *   missed      the samples whose first walk hits nothing
 *   backfacing  the samples whose first hit has dot(n, d) > 0.0f, n the shading normal at that hit: they see a surface from behind
 *
 * The basis.  Real SH on d = (x, y, z), fp32, in the association shown:
 *   Y0 = 0.282095f              Y1 = 0.488603f*y            Y2 = 0.488603f*z                          Y3 = 0.488603f*x
 *   Y4 = (1.092548f*x)*y        Y5 = (1.092548f*y)*z        Y6 = 0.315392f*((3.0f*(z*z)) - 1.0f)      Y7 = (1.092548f*x)*z
 *   Y8 = 0.546274f*((x*x) - (y*y))
 *
 * The record.  term_s[k][c] = Y_k(d_s) * L_s[c].  For j in 0..63, partial_j[k][c] = the fp32 sum from +0 of term_s[k][c] over
 * s = j, j + 64, j + 128, ... in increasing s (+0 where there is no such s).  sum[k][c] = (...((0 + partial_0) + partial_1) + ... +
 * partial_63).  sh[k][c] = (sum[k][c] * (4.0f * PT_PI_F)) / (float)samples.  The strided order is part of the definition: one wavefront
 * reduces one probe with coalesced loads and one ordered pass over its lanes.
 *
 * The lookup.  Given a grid, its count[0] * count[1] * count[2] probes -- probe (ix, iy, iz) has index (iz * ny + iy) * nx + ix and the
 * position origin[a] + (float)i_a * step[a] --, and a point (P, N) as pt_gather_points takes it.  Per axis a:
 *   g = (P[a] - origin[a]) / step[a];  g = fminf(fmaxf(g, 0.0f), (float)(count[a] - 1))   (a NaN coordinate lands on 0)
 *   i = min((int)floorf(g), count[a] - 2), i = 0 if count[a] == 1;  f = g - (float)i
 * The eight corners are taken x-fastest: corner c is (ix + (c & 1), iy + ((c >> 1) & 1), iz + (c >> 2)).  A corner's weight is
 * ((wx * wy) * wz), w = f on the upper side and 1.0f - f on the lower side.  The weight is 0 for a corner that does not exist (the upper
 * side of an axis with count 1; its term is formed with the lower side's record), and for a corner whose probe has
 * (float)backfacing > max_backfacing * (float)samples: such a probe sits inside geometry.  wsum = the sum of the eight weights in corner
 * order from +0.  If wsum == 0.0f the result is (0, 0, 0, 0).  Otherwise b[k][c] = (sum over the corners of w * sh_corner[k][c]) / wsum,
 * summed in corner order from +0 (all eight terms are formed: a weight of 0 does not hide a record that is not finite), and
 *   value[c] = fmaxf(sum over k = 0..8 of (a_k * Y_k(N)) * b[k][c], 0.0f), summed in k order from +0,
 *   a = (1.0f, 2.0f/3.0f x 3, 0.25f x 5)
 * -- the clamped-cosine convolution divided by pi: what a white Lambertian receiver at P that faces N sends out, the quantity
 * PT_GATHER_PATHS estimates.  The result is (value[0], value[1], value[2], wsum).
 *
 * Entry points.  The host forms take host memory and return when the results are there.  The _device forms take DEVICE pointers for
 * positions or probes and points, and for the results, and a hipStream_t, ordered as pt_gather_points_device orders its work; a null
 * stream makes the call wait.
 *   - pt_light_probes_points: n probes at positions[n][3].
 *   - pt_light_probes_grid: the probes of a grid; the positions are made on the device and never uploaded.
 *   - pt_light_probes_shade: the lookup for n points of six floats (position, normal); of `params` it reads max_backfacing alone.
 * The sampling is cut into launches of whole probes with at most PT_LIGHT_PROBE_CHUNK (an environment variable read per call; default
 * 2097152) (probe, sample) pairs each -- one probe where a probe alone has more --, over a workspace that is kept per device.
 *
 * Refusals, all before any device work and before the scene is locked, PT_ERR_INVALID: a null argument (n == 0 needs no arrays and
 * launches nothing), samples < 1, probes x samples above 0x7fffffff, an epsilon that is negative or NaN, a grid with a zero count, a step
 * that is zero or not finite, more than 0x7fffffff probes in a grid, a max_backfacing that is NaN or negative.  Every call holds the
 * scene's render lock, changes nothing in the scene, and is allowed with a live pt_frame and with or without a motion mark.
 *
 * Left out: bands above 2, visibility-weighted (Chebyshev) blending, more than one device, view batches, receivers other than white
 * Lambertian. */
#ifndef PT_LIGHT_PROBES_ABI_H
#define PT_LIGHT_PROBES_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_light_probe_params { int32_t samples; float epsilon; uint64_t base_seed; float max_backfacing; uint32_t pad; } pt_light_probe_params;
typedef struct pt_light_probe { float sh[9][3]; uint32_t samples, missed, backfacing; uint32_t pad[2]; } pt_light_probe; /* 128 bytes */
typedef struct pt_light_probe_grid { float origin[3]; float step[3]; uint32_t count[3]; } pt_light_probe_grid; /* probe (ix,iy,iz) has index (iz*ny+iy)*nx+ix */

/* 256 samples, epsilon 1e-3, base_seed 0, max_backfacing 0.25 */
int pt_light_probe_params_default(pt_light_probe_params *out);
int pt_light_probes_points(pt_scene *scene, const float *positions /* [n][3] */, size_t n, const pt_light_probe_params *params, pt_light_probe *out /* [n] */);
int pt_light_probes_points_device(pt_scene *scene, const float *d_positions, size_t n, const pt_light_probe_params *params, pt_light_probe *d_out, void *stream);
int pt_light_probes_grid(pt_scene *scene, const pt_light_probe_grid *grid, const pt_light_probe_params *params, pt_light_probe *out /* [nz][ny][nx] */);
int pt_light_probes_shade(pt_scene *scene, const pt_light_probe_grid *grid, const pt_light_probe *probes, const pt_light_probe_params *params,
                          const float *points /* [n][6]: position, normal */, size_t n, float *out /* [n][4] */);
int pt_light_probes_shade_device(pt_scene *scene, const pt_light_probe_grid *grid, const pt_light_probe *d_probes, const pt_light_probe_params *params,
                                 const float *d_points, size_t n, float *d_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
