// pt_relight.hip -- the device side of pt_scene_relight (pt_relight_kernels.h).
//
// The emitter registry (Scene::registerEmissiveObjects, reference src/scene/scene.cpp:183-208) is an ORDERED selection: the objects that
// emit, in the depth-first order of the tree's leaves.  It is made here by a stream compaction over that order -- a ballot per wavefront,
// a count per workgroup, one scan across the workgroups, and a second pass that writes every survivor at
//   survivors before its workgroup + survivors in the earlier wavefronts of the workgroup + survivors in the lower lanes of its wavefront
// -- so the order is kept by construction: no atomic counter, no sort.  Both passes are bound by the gathers through the order (the
// record's material word, nine floats of vertices for a candidate); position p is thread p, so the order, the ballots and the compacted
// outputs are read and written coalesced.
// Compiled with -ffp-contract=off and correctly rounded divide / sqrt like the rest: every operation is the IEEE operation of the host
// code in create_scene (pt_api.cpp), which this restates.
#include "pt_relight_kernels.h"
#include "pt_types.h"

namespace {

constexpr uint32_t WAVE = 64, WAVES = PT_RELIGHT_BLOCK / WAVE;
constexpr uint32_t SCAN_THREADS = 256; // (x PT_RELIGHT_BLOCK = 65,536 positions per trip of the scan's loop)
constexpr uint32_t PT_RELIGHT_NO_MATERIAL = 0xffffffffu; // PT_NO_MATERIAL of include/pt_hip.h

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    float d = 0.0f; // dot() starts from zero and adds in index order (detail/linear.h)
    d += ax * bx;
    d += ay * by;
    d += az * bz;
    return d;
}

// One object of the order as the registry sees it
struct Candidate {
    uint32_t ref;      // PT_REF_LEAF | triangle, or PT_REF_LEAF | PT_REF_SPHERE | sphere
    uint32_t material;
    uint32_t cull;
    float4 emission;
    float power, probability;
    bool registers;
};

// The reference, material and probability of object `obj`: create_scene's loop body up to the two tests (pt_api.cpp)
__device__ __forceinline__ Candidate candidate_of(const PtRelightScene &s, uint32_t obj) {
    Candidate c;
    c.ref = PT_REF_LEAF | (obj < s.n_desc_objects ? s.desc_ref[obj] : s.n_desc_tris + (obj - s.n_desc_objects));
    const uint32_t idx = c.ref & PT_REF_INDEX;
    const bool is_sphere = (c.ref & PT_REF_SPHERE) != 0u;
    c.cull = 0u;
    c.power = c.probability = 0.0f;
    c.emission = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    c.registers = false;
    if(is_sphere) {
        c.material = s.sph_meta[idx].x;
    }
    else {
        const float4 r2 = s.recs[PT_TRI_QUADS * static_cast<size_t>(idx) + 2];
        c.material = __float_as_uint(r2.y);
        c.cull = __float_as_uint(r2.z) >> 31;
    }
    if(c.material == PT_RELIGHT_NO_MATERIAL || c.material >= s.n_materials) {
        return c; // the default material has no emission (an index past the table cannot be: the host has checked every one)
    }
    c.emission = s.materials[4 * static_cast<size_t>(c.material) + 2];
    c.power = (c.emission.x + c.emission.y + c.emission.z) * c.emission.w;
    if(!(c.power > 0.0f)) {
        return c;
    }
    float area;
    if(is_sphere) {
        const float r = s.spheres[idx].w;
        area = 4.0f * 3.14159274101257324219f * (r * r); // object.cpp:95-99 (4.0F * pi is one constant on the host as well)
    }
    else {
        const float *p = s.tri_pos + 9 * static_cast<size_t>(idx);
        const float abx = p[3] - p[0], aby = p[4] - p[1], abz = p[5] - p[2];
        const float acx = p[6] - p[0], acy = p[7] - p[1], acz = p[8] - p[2];
        const float cx = aby * acz - abz * acy, cy = abz * acx - abx * acz, cz = abx * acy - aby * acx;
        area = __builtin_sqrtf(dot3(cx, cy, cz, cx, cy, cz)) / 2.0f; // object.cpp:188-190
    }
    c.probability = c.power * area;
    c.registers = c.probability > 0.0f;
    return c;
}

__global__ __launch_bounds__(PT_RELIGHT_BLOCK) void k_relight_flag(PtRelightScene s, unsigned long long *__restrict__ ballots, uint32_t *__restrict__ block_count,
                                                                  uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_count[WAVES];
    const uint32_t p = blockIdx.x * PT_RELIGHT_BLOCK + threadIdx.x, lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    bool registers = false, lit = false;
    if(p < s.n_objects) {
        const Candidate c = candidate_of(s, s.order[p]);
        registers = c.registers;
        lit = c.power > 0.0f;
    }
    const unsigned long long mask = __ballot(registers), lit_mask = __ballot(lit);
    if(lane == 0) {
        if(blockIdx.x * PT_RELIGHT_BLOCK + wave * WAVE < s.n_objects) {
            ballots[p / WAVE] = mask;
        }
        wave_count[wave] = static_cast<uint32_t>(__popcll(mask));
        if(lit_mask != 0ull) {
            atomicAdd(&counts[1], static_cast<uint32_t>(__popcll(lit_mask))); // (a count, not an order)
        }
    }
    __syncthreads();
    if(threadIdx.x == 0) {
        uint32_t sum = 0;
        for(uint32_t w = 0; w < WAVES; w++) {
            sum += wave_count[w];
        }
        block_count[blockIdx.x] = sum;
    }
}

// block_first[b] = the sum of block_first[0 .. b - 1] (in place), counts[0] = the sum of all: one workgroup walks the array in chunks of
// its size with a running carry
__global__ __launch_bounds__(SCAN_THREADS) void k_relight_scan(uint32_t *__restrict__ block_first, uint32_t n_blocks, uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_sum[SCAN_THREADS / WAVE];
    __shared__ uint32_t carry;
    const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if(threadIdx.x == 0) {
        carry = 0;
    }
    __syncthreads();
    for(uint32_t base = 0; base < n_blocks; base += SCAN_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? block_first[i] : 0u;
        uint32_t incl = v; // inclusive scan inside the wavefront
        for(uint32_t d = 1; d < WAVE; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, WAVE);
            if(lane >= d) {
                incl += up;
            }
        }
        if(lane == WAVE - 1) {
            wave_sum[wave] = incl;
        }
        __syncthreads();
        uint32_t before = carry;
        for(uint32_t w = 0; w < wave; w++) {
            before += wave_sum[w];
        }
        if(i < n_blocks) {
            block_first[i] = before + incl - v;
        }
        __syncthreads();
        if(threadIdx.x == SCAN_THREADS - 1) {
            carry = before + incl;
        }
        __syncthreads();
    }
    if(threadIdx.x == 0) {
        counts[0] = carry;
    }
}

__global__ __launch_bounds__(PT_RELIGHT_BLOCK) void k_relight_emit(PtRelightScene s, const unsigned long long *__restrict__ ballots, const uint32_t *__restrict__ block_first,
                                                                  float4 *__restrict__ emis, float *__restrict__ prob, uint32_t *__restrict__ out_obj) {
    const uint32_t p = blockIdx.x * PT_RELIGHT_BLOCK + threadIdx.x, lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if(p >= s.n_objects) {
        return;
    }
    const uint32_t first_word = blockIdx.x * WAVES; // (every word up to this position's own exists: its wavefront holds a position < n_objects)
    const unsigned long long mask = ballots[first_word + wave];
    if(((mask >> lane) & 1ull) == 0ull) {
        return;
    }
    uint32_t k = block_first[blockIdx.x] + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
    for(uint32_t w = 0; w < wave; w++) {
        k += static_cast<uint32_t>(__popcll(ballots[first_word + w]));
    }
    const uint32_t obj = s.order[p];
    const Candidate c = candidate_of(s, obj);
    const uint32_t idx = c.ref & PT_REF_INDEX;
    float4 *e = emis + 4 * static_cast<size_t>(k);
    if((c.ref & PT_REF_SPHERE) != 0u) {
        e[0] = s.spheres[idx];
        e[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        e[2] = make_float4(0.0f, __uint_as_float(c.ref), 0.0f, __uint_as_float(c.material));
    }
    else {
        const float *v = s.tri_pos + 9 * static_cast<size_t>(idx);
        e[0] = make_float4(v[0], v[1], v[2], v[3]);
        e[1] = make_float4(v[4], v[5], v[6], v[7]);
        e[2] = make_float4(v[8], __uint_as_float(c.ref), __uint_as_float(c.cull), __uint_as_float(c.material));
    }
    e[3] = c.emission;
    prob[k] = c.probability;
    out_obj[k] = obj;
}

// Thread j is the j-th triangle of the ranges laid end to end (range r starts at ranges[r].pad)
__global__ __launch_bounds__(256) void k_relight_materials(const PtRelightRange *__restrict__ ranges, uint32_t n_ranges, uint32_t total, float4 *__restrict__ recs,
                                                          float4 *__restrict__ tri_shade) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if(j >= total) {
        return;
    }
    uint32_t lo = 0, hi = n_ranges; // the last range that starts at or before j
    while(hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if(ranges[mid].pad <= j) {
            lo = mid;
        }
        else {
            hi = mid;
        }
    }
    const PtRelightRange r = ranges[lo];
    const uint32_t k = j - r.pad;
    if(k >= r.count) {
        return;
    }
    const size_t t = static_cast<size_t>(r.first_tri) + k;
    reinterpret_cast<uint32_t *>(recs + PT_TRI_QUADS * t + 2)[1] = r.material;
    reinterpret_cast<uint32_t *>(tri_shade + 8 * t + 2)[1] = r.material;
}

} // namespace

hipError_t pt_relight_flag(hipStream_t stream, const PtRelightScene &scene, unsigned long long *ballots, uint32_t *block_first, uint32_t *counts) {
    hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), stream);
    if(e != hipSuccess || scene.n_objects == 0) {
        return e;
    }
    const uint32_t n_blocks = pt_relight_blocks(scene.n_objects);
    hipLaunchKernelGGL(k_relight_flag, dim3(n_blocks), dim3(PT_RELIGHT_BLOCK), 0, stream, scene, ballots, block_first, counts);
    hipLaunchKernelGGL(k_relight_scan, dim3(1), dim3(SCAN_THREADS), 0, stream, block_first, n_blocks, counts);
    return hipGetLastError();
}

hipError_t pt_relight_emit(hipStream_t stream, const PtRelightScene &scene, const unsigned long long *ballots, const uint32_t *block_first, float4 *emis, float *prob,
                           uint32_t *obj) {
    if(scene.n_objects == 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_relight_emit, dim3(pt_relight_blocks(scene.n_objects)), dim3(PT_RELIGHT_BLOCK), 0, stream, scene, ballots, block_first, emis, prob, obj);
    return hipGetLastError();
}

hipError_t pt_relight_materials(hipStream_t stream, const PtRelightRange *ranges, uint32_t n_ranges, uint32_t total, float4 *recs, float4 *tri_shade) {
    if(n_ranges == 0 || total == 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_relight_materials, dim3((total + 255) / 256), dim3(256), 0, stream, ranges, n_ranges, total, recs, tri_shade);
    return hipGetLastError();
}
