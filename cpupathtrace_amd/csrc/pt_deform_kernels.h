// pt_deform_kernels.h -- the skinning kernel and its launch (pt_skin.h; include/pt_deform.h): linear blend skinning of
// one mesh's rest vertices, one thread per vertex, 256 per block like the assembler's kernels.  Included once, by pt_deform.hip;
// tests/hip/deform_probe.hip includes it as well and, compiled for the host, runs this very source on the CPU.
//
// Vertex i = (x, y, z), component c of its result:
//     acc = 0
//     for k = 0 .. K-1, in order:   B = bones[bone[i][k]]
//                                   d = 0;  d += B[c][0] * x;  d += B[c][1] * y;  d += B[c][2] * z;  d += B[c][3] * 1     (kb_transform's dot)
//                                   acc += weight[i][k] * d
// Every product and every sum is an IEEE float operation of its own (-ffp-contract=off), so the result has one bit pattern.  No
// influence is skipped -- a zero weight on a bone with an infinite or NaN entry gives NaN --, no weight is normalised, nothing is divided.
// No bone index is checked: pt_scene_bind_skin has checked them all on the host.
//
// Traffic per vertex: 12 bytes of rest vertex, 4 * K of indices and 4 * K of weights read, 12 written: 24 + 8 * K, plus the bone table.
// A vertex's K indices (and K weights) are 4 * K contiguous bytes at a multiple of 4 * K: they are read with the widest load that
// alignment allows, 16 bytes for K = 4 and 8, 8 bytes for K = 2 and 6, 4 bytes for an odd K.  The bone table (48 bytes per bone, read as
// three float4) has two forms, chosen per launch (PT_SKIN_LDS_BONES, pt_skin.h): staged in LDS by the whole block, or read through the
// cache.  Threads past the last vertex take part in the staging and in the barrier.  Indices are 64-bit where 3 * i or K * i can pass 2^32.
#ifndef PT_DEFORM_KERNELS_H
#define PT_DEFORM_KERNELS_H

#include "pt_skin.h"

namespace ptsk {

// N consecutive 4-byte items, aligned as a whole
template<typename T, int N>
struct alignas(4 * N) Pack {
    T v[N];
};

template<typename T, int K>
__device__ __forceinline__ void load_row(const T *__restrict__ base, size_t i, T (&out)[K]) {
    constexpr int W = K % 4 == 0 ? 4 : (K % 2 == 0 ? 2 : 1);
    const Pack<T, W> *p = reinterpret_cast<const Pack<T, W> *>(base + static_cast<size_t>(K) * i);
    for(int j = 0; j < K / W; j++) {
        const Pack<T, W> q = p[j];
        for(int e = 0; e < W; e++) {
            out[W * j + e] = q.v[e];
        }
    }
}

__device__ __forceinline__ float row_dot(const float4 &r, float x, float y, float z) {
    float d = 0.0f;
    d += r.x * x;
    d += r.y * y;
    d += r.z * z;
    d += r.w * 1.0f;
    return d;
}

template<int K, bool LDS>
__global__ void __launch_bounds__(256) kd_skin(uint32_t n_vertices, const float *__restrict__ rest, const uint32_t *__restrict__ bone, const float *__restrict__ weight,
                                               const float4 *__restrict__ bones, uint32_t n_bones, float *__restrict__ out) {
    __shared__ float4 staged[LDS ? 3 * PT_SKIN_LDS_BONES : 1];
    if constexpr(LDS) {
        for(uint32_t e = threadIdx.x; e < 3 * n_bones; e += 256u) {
            staged[e] = bones[e];
        }
        __syncthreads();
    }
    const uint64_t i64 = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if(i64 >= n_vertices) {
        return;
    }
    const size_t i = static_cast<size_t>(i64);
    const float x = rest[3 * i], y = rest[3 * i + 1], z = rest[3 * i + 2];
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
            const float d = row_dot(r[c], x, y, z);
            acc[c] += w[k] * d;
        }
    }
    out[3 * i] = acc[0];
    out[3 * i + 1] = acc[1];
    out[3 * i + 2] = acc[2];
}

template<int K>
void launch(hipStream_t stream, bool lds, uint32_t n_vertices, const float *rest, const uint32_t *bone, const float *weight, const float4 *bones, uint32_t n_bones, float *out) {
    const dim3 grid(static_cast<unsigned>((static_cast<uint64_t>(n_vertices) + 255) / 256));
    if(lds) {
        hipLaunchKernelGGL((kd_skin<K, true>), grid, dim3(256), 0, stream, n_vertices, rest, bone, weight, bones, n_bones, out);
    }
    else {
        hipLaunchKernelGGL((kd_skin<K, false>), grid, dim3(256), 0, stream, n_vertices, rest, bone, weight, bones, n_bones, out);
    }
}

} // namespace ptsk

hipError_t pt_skin_launch(hipStream_t stream, uint32_t n_vertices, const float *rest, uint32_t K, const uint32_t *bone, const float *weight, const float *bones,
                          uint32_t n_bones, uint32_t lds_bones, float *out) {
    if(K < 1 || K > PT_SKIN_MAX_K || n_bones == 0) {
        return hipErrorInvalidValue;
    }
    if(n_vertices == 0) {
        return hipSuccess;
    }
    const bool lds = n_bones <= (lds_bones < PT_SKIN_LDS_BONES ? lds_bones : PT_SKIN_LDS_BONES);
    const float4 *table = reinterpret_cast<const float4 *>(bones);
    switch(K) {
    case 1: ptsk::launch<1>(stream, lds, n_vertices, rest, bone, weight, table, n_bones, out); break;
    case 2: ptsk::launch<2>(stream, lds, n_vertices, rest, bone, weight, table, n_bones, out); break;
    case 3: ptsk::launch<3>(stream, lds, n_vertices, rest, bone, weight, table, n_bones, out); break;
    case 4: ptsk::launch<4>(stream, lds, n_vertices, rest, bone, weight, table, n_bones, out); break;
    case 5: ptsk::launch<5>(stream, lds, n_vertices, rest, bone, weight, table, n_bones, out); break;
    case 6: ptsk::launch<6>(stream, lds, n_vertices, rest, bone, weight, table, n_bones, out); break;
    case 7: ptsk::launch<7>(stream, lds, n_vertices, rest, bone, weight, table, n_bones, out); break;
    default: ptsk::launch<8>(stream, lds, n_vertices, rest, bone, weight, table, n_bones, out); break;
    }
    return hipGetLastError();
}

#endif
