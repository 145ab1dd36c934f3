/* pt_light_passes.h -- light-group passes: the radiance of pt_radiance.h's rays and captures split by the emitter group a term came from
 * and, optionally, by how often the path had scattered before it -- so that a caller traces once and then turns single lights up, down or
 * to another colour without tracing again.
 * Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h reaches this file through pt_radiance.h, whose last line includes it; it is
 * not meant to be included on its own.
 *
 * Radiance is linear in the emitters.  A call takes `samples` samples of every ray, or of every pixel of a capture, exactly as the
 * radiance calls do, and returns P = n_groups * (split ? 3 : 1) 16-byte pt_light_pass records each -- [n][P], or [height][width][P] --
 * and, where `total` is not NULL, the 32-byte pt_radiance_result the radiance call returns for the same arguments.
 *
 * The sample.  Engines, the first ray, the capture generators, the jitter draws and the `outside` samples are pt_radiance.h's: sample s
 * of ray or pixel i has the engine RandomEngine(pt_pixel_seed(base_seed, x = s, y = i)), and the path behind the ray is getSample's, draw
 * for draw.  The group table changes no draw and no decision.
 *
 * Every addition carries a pass.  Every term the reference adds to out_spectrum is also added, as its rgb, to exactly one pass
 * accumulator: p = group * C + component, C = split ? 3 : 1, component = 0 when split == 0.
 *   the emission term of a vertex (worker.cpp:62-64): group = material_group[the vertex's material], PT_NO_MATERIAL has group 0; the
 *     scatterings are k = path_length - 1, path_length taken after its increment
 *   a light sample at a vertex (worker.cpp:76-103): for point light j, group = point_light_group[j]; for an emitter sample, group =
 *     material_group[the material of the registry object the sample chose] -- the object_index of Scene::sampleLights, scene.cpp:238-286;
 *     the scatterings are k = path_length
 *   component = min(k, 2): PT_PASS_EMITTED, the light source seen along the ray itself; PT_PASS_DIRECT, one scattering -- the light
 *     samples at the first vertex and the emission a bounce ray finds at the second: the reference counts both, and so does this split;
 *     PT_PASS_INDIRECT, everything else.
 *
 * Each accumulator starts at (+0, +0, +0) and takes acc = acc + term in fp32, in the order in which the path makes the terms.  (A term
 * that is all zeros is skipped on the device: an accumulator is never -0, so adding +-0 changes no bit.)
 *
 * The record.  Each pass of each ray or pixel is reduced over its samples in pt_radiance.h's strided order: for j in 0..63, partial_j =
 * the fp32 sum from +0 of the sample's accumulator over s = j, j + 64, ... in increasing s; sum = (...((0 + partial_0) + partial_1) +
 * ... + partial_63); value = sum / (float)samples; pad = 0.  A sample that missed, or that has no ray, contributes zeros to every pass.
 * total[i] is the record of the radiance call for the same scene, rays or capture and parameters, bit for bit -- value, alpha, samples,
 * missed, outside: it comes from the ordinary accumulator, which is kept beside the passes.  The passes of a ray do NOT in general add
 * up to total bit for bit: the same terms are added in another association.  With one group, split == 0 and samples == 1 they do: the
 * single accumulator takes the terms the ordinary one takes, in its order.
 *
 * The mix.  out[i][c] = (...((+0 + passes[i][0].value[c] * gains[0][c]) + passes[i][1].value[c] * gains[1][c]) + ...) over the n_passes
 * passes, c = 0..2, in fp32, each product rounded before it is added.  out[i][3] = total[i].value[3] where total is given, else 0.  Any
 * gain, finite or not, is taken as given.  pt_light_passes_mix computes on the host, from host memory, and needs no device;
 * pt_light_passes_mix_device takes DEVICE pointers for everything and runs one thread per ray or pixel on the scene's device.
 *
 * Entry points.  The host forms take host memory and return when the results are there.  The _device forms take DEVICE pointers for the
 * rays, the passes and the total -- the group tables stay in host memory and are read before the call returns -- and a hipStream_t,
 * ordered as the radiance calls' device forms order their work; a null stream makes the call wait.  The work is cut into launches of
 * whole rays or pixels with at most PT_RADIANCE_CHUNK / P (ray or pixel, sample) pairs each -- the variable pt_radiance.h reads, per call
 * -- and at least one ray or pixel, over a workspace that is kept per device: one 16-byte cell per (pass, pair) and one per pair for the
 * total, and the two group tables, uploaded per call.  A record depends on neither chunking nor launch shape.
 *
 * Refusals before any device work and before the scene is locked, PT_ERR_INVALID, in this order: every refusal of the corresponding
 * radiance call; null `groups` or `passes` (n == 0 needs no arrays but it needs `groups`); n_groups outside 1..8; a split other than 0
 * or 1; a null table with a non-zero count; a table entry >= n_groups; rays x samples x P or pixels x samples x P above 0x7fffffff.
 * The mix: a null argument with n > 0 (total may always be NULL), n_passes outside 1..24.  Under the scene's lock, before any launch,
 * PT_ERR_INVALID: n_materials or n_point_lights different from the scene's current counts -- a table made before a pt_scene_relight
 * cannot be applied to the new look by accident.  Every call changes nothing in the scene and is allowed with a live pt_frame and with
 * or without a motion mark.
 *
 * Left out: a pinhole or thin-lens model (callers pass their own rays), adaptive sampling, resumable and checkpointed passes,
 * per-instance groups (groups follow materials), denoising of passes, more than one device. */
#ifndef PT_LIGHT_PASSES_ABI_H
#define PT_LIGHT_PASSES_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

#define PT_LIGHT_GROUPS_MAX 8
#define PT_PASS_EMITTED  0
#define PT_PASS_DIRECT   1
#define PT_PASS_INDIRECT 2

typedef struct pt_light_groups {
    uint32_t n_groups;                /* 1..8 */
    int32_t split;                    /* 0: one pass per group; 1: three per group (emitted, direct, indirect) */
    const uint8_t *material_group;    /* [n_materials]: the group of every material of the scene's table */
    uint32_t n_materials;
    const uint8_t *point_light_group; /* [n_point_lights] */
    uint32_t n_point_lights;
} pt_light_groups; /* 40 bytes */

typedef struct pt_light_pass { float value[3]; uint32_t pad; } pt_light_pass; /* 16 bytes, pad = 0 */

/* *n_passes = P = n_groups * (split ? 3 : 1); refuses what the calls below refuse of n_groups and split */
int pt_light_passes_count(const pt_light_groups *groups, uint32_t *n_passes);
int pt_light_passes_rays(pt_scene *scene, const float *rays /* [n][6] */, size_t n, const pt_light_groups *groups, const pt_radiance_params *params, pt_light_pass *passes /* [n][P] */,
                         pt_radiance_result *total /* [n], may be NULL */);
int pt_light_passes_rays_device(pt_scene *scene, const float *d_rays, size_t n, const pt_light_groups *groups, const pt_radiance_params *params, pt_light_pass *d_passes,
                                pt_radiance_result *d_total, void *stream);
int pt_light_passes_capture(pt_scene *scene, const pt_capture_desc *capture, const pt_light_groups *groups, const pt_radiance_params *params,
                            pt_light_pass *passes /* [height][width][P] */, pt_radiance_result *total /* [height][width], may be NULL */);
int pt_light_passes_capture_device(pt_scene *scene, const pt_capture_desc *capture, const pt_light_groups *groups, const pt_radiance_params *params, pt_light_pass *d_passes,
                                   pt_radiance_result *d_total, void *stream);
int pt_light_passes_mix(const pt_light_pass *passes /* [n][n_passes] */, size_t n, uint32_t n_passes, const float *gains /* [n_passes][3] */,
                        const pt_radiance_result *total /* [n], may be NULL */, float *out /* [n][4] */);
int pt_light_passes_mix_device(pt_scene *scene /* for its device and stream */, const pt_light_pass *d_passes, size_t n, uint32_t n_passes, const float *d_gains,
                               const pt_radiance_result *d_total, float *d_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
