// pt_skin.h -- linear blend skinning of a mesh's rest vertices on the device (pt_deform.hip, kernels in pt_deform_kernels.h, where the
// arithmetic and the two forms of the bone table are described; include/pt_deform.h).
#ifndef PT_SKIN_H
#define PT_SKIN_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

// The most influences per vertex (PT_SKIN_MAX_INFLUENCES of include/pt_deform.h)
#define PT_SKIN_MAX_K 8

// The largest bone table a block stages in LDS: 256 bones of 48 bytes, 12 KiB.  Two bounds meet here.  Occupancy: a block of 256 threads
// is 4 wavefronts and a CU holds 32, so 8 blocks share its 160 KiB of LDS, 20 KiB each; 12 KiB keeps all 8 resident.  Traffic: staging
// reads 48 * n_bones bytes per block in whole lines, the cache form gathers 256 * K records of 48 bytes per block in 16-byte pieces;
// beyond 256 bones a block of K = 1 would stage more than it gathers.  Larger tables are read through the cache.
#define PT_SKIN_LDS_BONES 256u

// out[i] = sum over k < K, in order, of weight[i][k] * (bones[bone[i][k]] * (rest[i], 1)) for the n_vertices vertices of one mesh, one
// launch on `stream`.  rest / out: [n_vertices][3]; bone / weight: [n_vertices][K], 16-byte aligned at row 0; bones: [n_bones][12], rows
// 0 .. 2 of each mat4, 16-byte aligned.  Every bone[i][k] must be < n_bones: the kernel checks none.  The table is staged in LDS when
// n_bones <= min(lds_bones, PT_SKIN_LDS_BONES) and read through the cache otherwise (lds_bones = 0 forces that form).
// hipErrorInvalidValue for K outside 1 .. PT_SKIN_MAX_K or n_bones == 0.
hipError_t pt_skin_launch(hipStream_t stream, uint32_t n_vertices, const float *rest, uint32_t K, const uint32_t *bone, const float *weight, const float *bones,
                          uint32_t n_bones, uint32_t lds_bones, float *out);

#endif
