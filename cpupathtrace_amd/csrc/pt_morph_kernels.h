// pt_morph_kernels.h -- the blend-shape kernel and its launch (pt_morph_skin.h; include/pt_morph.h): the morph of one
// mesh's rest vertices, alone (K = 0) or fused with linear blend skinning (K = 1 .. 8), one thread per vertex, 256 per block like
// kd_skin.  Included once, by pt_deform.hip, behind pt_deform_kernels.h, whose load_row and row_dot it uses: the two headers share that
// translation unit so that pt_skin_launch has one definition.  tests/hip/morph_probe.hip includes it as well and, compiled for the
// host, runs this very source on the CPU.
//
// Vertex i, component c:
//     m = rest[i][c]
//     for e = row_start[i] .. row_start[i + 1] - 1, in order:   m += weights[entries[e].target] * entries[e].d[c]
// The rows are vertex-major and hold a vertex's entries in ascending target order (pt_scene_bind_morphs sorts them so on the host): a
// gather with one fixed order of summation, where a scatter with atomics would have none.  Product and sum are IEEE float operations
// of their own (-ffp-contract=off), no entry is skipped -- a zero weight on an infinite or NaN delta gives NaN, and on any delta turns a
// rest component of -0.0 into +0.0 --, no weight is clamped or normalised.  With K >= 1 the morphed vertex stays in registers and takes
// the place of the rest vertex in kd_skin's arithmetic (pt_deform_kernels.h), operation for operation.  No index is checked:
// pt_scene_bind_morphs and pt_scene_bind_skin have checked them all on the host.
//
// Traffic per vertex: 12 bytes of rest vertex, 4 of row_start (the neighbour's end is the next lane's start), 16 per entry, 8 * K of
// indices and weights, 12 written: 28 + 16 * entries + 8 * K, plus the tables.  An entry is one 16-byte load at a multiple of 16.  The
// lanes of a wavefront diverge only by the lengths of their rows: a row's sum is sequential by definition, so there is nothing to split
// across lanes.  The weights (and with K >= 1 the bone table) have two forms, chosen per launch (PT_MORPH_LDS_TARGETS, pt_morph_skin.h):
// staged in LDS by the whole block behind ONE barrier, or read through the cache.  Threads past the last vertex take part in the
// staging and in the barrier.  Indices are 64-bit where 3 * i, K * i or an entry's offset can pass 2^32.
#ifndef PT_MORPH_KERNELS_H
#define PT_MORPH_KERNELS_H

#include "pt_deform_kernels.h"
#include "pt_morph_skin.h"

namespace ptsk {

template<int K, bool LDS>
__global__ void __launch_bounds__(256) kd_morph(uint32_t n_vertices, const float *__restrict__ rest, const uint32_t *__restrict__ row_start,
                                                const PtMorphEntry *__restrict__ entries, const float *__restrict__ weights, uint32_t n_targets,
                                                const uint32_t *__restrict__ bone, const float *__restrict__ weight, const float4 *__restrict__ bones, uint32_t n_bones,
                                                float *__restrict__ out) {
    __shared__ float staged_weights[LDS ? PT_MORPH_LDS_TARGETS : 1];
    __shared__ float4 staged[LDS && K > 0 ? 3 * PT_SKIN_LDS_BONES : 1];
    if constexpr(LDS) {
        for(uint32_t t = threadIdx.x; t < n_targets; t += 256u) {
            staged_weights[t] = weights[t];
        }
        if constexpr(K > 0) {
            for(uint32_t e = threadIdx.x; e < 3 * n_bones; e += 256u) {
                staged[e] = bones[e];
            }
        }
        __syncthreads();
    }
    const uint64_t i64 = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if(i64 >= n_vertices) {
        return;
    }
    const size_t i = static_cast<size_t>(i64);
    float m[3] = {rest[3 * i], rest[3 * i + 1], rest[3 * i + 2]};
    const size_t row_end = row_start[i + 1];
    for(size_t e = row_start[i]; e < row_end; e++) {
        const PtMorphEntry entry = entries[e];
        float w;
        if constexpr(LDS) {
            w = staged_weights[entry.target];
        }
        else {
            w = weights[entry.target];
        }
        m[0] += w * entry.dx;
        m[1] += w * entry.dy;
        m[2] += w * entry.dz;
    }
    if constexpr(K > 0) {
        uint32_t b[K];
        float w[K];
        load_row<uint32_t, K>(bone, i, b);
        load_row<float, K>(weight, i, w);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for(int k = 0; k < K; k++) {
            float4 r[3];
            for(int c = 0; c < 3; c++) {
                if constexpr(LDS) {
                    r[c] = staged[3 * b[k] + c];
                }
                else {
                    r[c] = bones[3 * static_cast<size_t>(b[k]) + c];
                }
            }
            for(int c = 0; c < 3; c++) {
                const float d = row_dot(r[c], m[0], m[1], m[2]);
                acc[c] += w[k] * d;
            }
        }
        m[0] = acc[0];
        m[1] = acc[1];
        m[2] = acc[2];
    }
    out[3 * i] = m[0];
    out[3 * i + 1] = m[1];
    out[3 * i + 2] = m[2];
}

template<int K>
void launch_morph(hipStream_t stream, bool lds, uint32_t n_vertices, const float *rest, const uint32_t *row_start, const PtMorphEntry *entries, const float *weights,
                  uint32_t n_targets, const uint32_t *bone, const float *weight, const float4 *bones, uint32_t n_bones, float *out) {
    const dim3 grid(static_cast<unsigned>((static_cast<uint64_t>(n_vertices) + 255) / 256));
    if(lds) {
        hipLaunchKernelGGL((kd_morph<K, true>), grid, dim3(256), 0, stream, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, bones, n_bones, out);
    }
    else {
        hipLaunchKernelGGL((kd_morph<K, false>), grid, dim3(256), 0, stream, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, bones, n_bones, out);
    }
}

} // namespace ptsk

hipError_t pt_morph_launch(hipStream_t stream, uint32_t n_vertices, const float *rest, const uint32_t *row_start, const PtMorphEntry *entries, const float *weights,
                           uint32_t n_targets, uint32_t lds_targets, uint32_t K, const uint32_t *bone, const float *weight, const float *bones, uint32_t n_bones,
                           uint32_t lds_bones, float *out) {
    if(K > PT_SKIN_MAX_K || n_targets == 0 || (K > 0 && n_bones == 0)) {
        return hipErrorInvalidValue;
    }
    if(n_vertices == 0) {
        return hipSuccess;
    }
    const bool weights_fit = n_targets <= (lds_targets < PT_MORPH_LDS_TARGETS ? lds_targets : PT_MORPH_LDS_TARGETS);
    const bool bones_fit = K == 0 || n_bones <= (lds_bones < PT_SKIN_LDS_BONES ? lds_bones : PT_SKIN_LDS_BONES);
    const bool lds = weights_fit && bones_fit;
    const float4 *table = reinterpret_cast<const float4 *>(bones);
    switch(K) {
    case 0: ptsk::launch_morph<0>(stream, lds, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, table, n_bones, out); break;
    case 1: ptsk::launch_morph<1>(stream, lds, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, table, n_bones, out); break;
    case 2: ptsk::launch_morph<2>(stream, lds, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, table, n_bones, out); break;
    case 3: ptsk::launch_morph<3>(stream, lds, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, table, n_bones, out); break;
    case 4: ptsk::launch_morph<4>(stream, lds, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, table, n_bones, out); break;
    case 5: ptsk::launch_morph<5>(stream, lds, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, table, n_bones, out); break;
    case 6: ptsk::launch_morph<6>(stream, lds, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, table, n_bones, out); break;
    case 7: ptsk::launch_morph<7>(stream, lds, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, table, n_bones, out); break;
    default: ptsk::launch_morph<8>(stream, lds, n_vertices, rest, row_start, entries, weights, n_targets, bone, weight, table, n_bones, out); break;
    }
    return hipGetLastError();
}

#endif
