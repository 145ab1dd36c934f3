// pt_morph_skin.h -- blend shapes of a mesh's rest vertices on the device, alone or in front of linear blend skinning (pt_deform.hip,
// kernel in pt_morph_kernels.h, where the arithmetic and the two forms of the tables are described; include/pt_morph.h).
#ifndef PT_MORPH_SKIN_H
#define PT_MORPH_SKIN_H

#include "pt_skin.h"

// One delta of one target on one vertex, in the vertex-major table pt_scene_bind_morphs builds on the host: 16 bytes at a multiple of
// 16, so that the kernel reads an entry with a single 16-byte load.
struct alignas(16) PtMorphEntry {
    float dx, dy, dz;
    uint32_t target;
};

// The most weights a block stages in LDS: 2048 floats, 8 KiB.  pt_skin.h derives 20 KiB of LDS per block of 256 threads at full
// occupancy (8 blocks share a CU's 160 KiB); the bone table of a fused launch takes 12 KiB of them (PT_SKIN_LDS_BONES), which leaves
// 8 KiB.  Staging reads 4 * n_targets bytes per block in whole lines; sets with more targets read their weights through the cache.
#define PT_MORPH_LDS_TARGETS 2048u

// out[i] = skin(morph(rest[i])) for the n_vertices vertices of one mesh, one launch on `stream`:
//     m = rest[i];  for e = row_start[i] .. row_start[i + 1] - 1, in order:  m[c] += weights[entries[e].target] * entries[e].d[c]
// and, with K >= 1, m instead of the rest vertex through pt_skin_launch's arithmetic (K = 0: out[i] = m; bone, weight and bones are not
// read).  rest / out: [n_vertices][3]; row_start: [n_vertices + 1], ascending; entries: 16-byte aligned, every target < n_targets;
// weights: [n_targets]; bone / weight / bones as pt_skin_launch takes them.  The kernel checks no index.  Weights and bone table are
// staged in LDS together when n_targets <= min(lds_targets, PT_MORPH_LDS_TARGETS) and (K = 0 or) n_bones <= min(lds_bones,
// PT_SKIN_LDS_BONES), and both read through the cache otherwise.  hipErrorInvalidValue for K > PT_SKIN_MAX_K, n_targets == 0, or
// K >= 1 with n_bones == 0.
hipError_t pt_morph_launch(hipStream_t stream, uint32_t n_vertices, const float *rest, const uint32_t *row_start, const PtMorphEntry *entries, const float *weights,
                           uint32_t n_targets, uint32_t lds_targets, uint32_t K, const uint32_t *bone, const float *weight, const float *bones, uint32_t n_bones,
                           uint32_t lds_bones, float *out);

#endif
