// pt_light_pass_kernels.h -- light-group passes (include/pt_light_passes.h): the kernel that traces the samples of a chunk
// of rays or pixels and keeps an accumulator per pass beside the ordinary one, the reduction that makes the pass records, and the mix.
// Included by exactly one translation unit, pt_walks.hip, behind pt_sample_walk.h and pt_radiance_kernels.h, and so behind capture_ray,
// RadianceSink, bind_lane and dispatch_route.
//
// The sample is the shared loop's (sample_walk, pt_sample_walk.h) behind pt_radiance_sample_kernel's first ray; what this kernel adds to it
// is a sink that asks for every term's emitter and sends the term, at each of the loop's three addition sites, to the lane's cell of one
// pass as well.  The accumulators live in the chunk's workspace, pass-major -- passes[p * n_pairs + pair], 16 bytes each --, not in
// registers: 24 passes would be 72 VGPRs on top of a loop that already carries the tracer.  The 64 lanes of a wavefront touch 64
// neighbouring cells; a lane reads, adds and writes only its own cell with plain vector loads and stores, so no atomics are needed, and
// it zeroes its P cells before its loop.
#ifndef PT_LIGHT_PASS_KERNELS_H
#define PT_LIGHT_PASS_KERNELS_H

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_shading.h"

namespace {

using namespace ptd;

// groups[material] (PT_NO_MATERIAL: group 0); the table holds the materials' groups, then the point lights'
PT_D uint32_t material_group(const uint8_t *__restrict__ groups, uint32_t material) {
    return material == 0xFFFFFFFFu ? 0u : (uint32_t)groups[material];
}

// cell = cell + term (rgb) for the lane's cell of a pass; a term of zeros changes no bit of a cell that is never -0, and most vertices
// emit nothing: no traffic for them
PT_D void pass_add(float4 *__restrict__ cell, const C4 &term) {
    if(term.r == 0.0f && term.g == 0.0f && term.b == 0.0f) {
        return;
    }
    float4 v = *cell;
    v.x = v.x + term.r;
    v.y = v.y + term.g;
    v.z = v.z + term.b;
    *cell = v;
}

// The radiance sink that also splits: an emitter is kept as its group, and a term goes to the cell of pass group * per_group + depth,
// depth = min(scatterings before the term, 2) where the call splits by depth
struct LightPassSink : RadianceSink {
    static constexpr bool kEmitters = true;
    typedef uint32_t Emitter;
    const uint8_t *__restrict__ groups;
    uint32_t n_materials, per_group, split;
    float4 *__restrict__ mine; // pass p: mine[p * n_pairs]
    uint32_t n_pairs;
    PT_D Emitter point_light(uint32_t j) const { return (uint32_t)groups[n_materials + j]; }
    PT_D Emitter material(uint32_t m) const { return material_group(groups, m); }
    PT_D void add(const C4 &term, uint32_t group, int scatterings) {
        pass_add(mine + (size_t)(group * per_group + (split != 0u ? (uint32_t)(scatterings < 2 ? scatterings : 2) : 0u)) * n_pairs, term);
    }
    PT_D void direct(const C4 &term, Emitter group, int path_length) { add(term, group, path_length); }
    PT_D void emitted(const C4 &term, Emitter group, int path_length) { add(term, group, path_length - 1); }
};

// The samples of the rays or pixels first .. first + n_pairs / samples - 1: plane[g] as pt_radiance_sample_kernel leaves it, and
// passes[p * n_pairs + g] = (the pass's rgb, 0) for p < n_groups * (split ? 3 : 1).  groups: the materials' groups, then, from
// n_materials on, the point lights'.
template<int STACK_LDS, bool IN_LDS>
__global__ __launch_bounds__(256) void pt_light_pass_sample_kernel(PtDevScene sc, const float *__restrict__ rays, PtCaptureParams cap, uint32_t first, uint32_t samples, uint32_t n_pairs,
                                                                   float epsilon, uint64_t base_seed, const uint8_t *__restrict__ groups, uint32_t n_materials, uint32_t n_passes,
                                                                   uint32_t split, float4 *__restrict__ plane, float4 *__restrict__ passes, uint2 *__restrict__ spill,
                                                                   uint32_t spill_depth) {
    Tracer<STACK_LDS, IN_LDS> tr;
    const size_t gid = bind_lane(tr, sc, spill, spill_depth);
    if(gid >= n_pairs) {
        return;
    }
    const uint32_t local = (uint32_t)gid / samples;
    const uint32_t sample = (uint32_t)gid - local * samples;
    const uint32_t index = first + local;
    float4 *__restrict__ mine = passes + gid; // pass p: mine[p * n_pairs]
    for(uint32_t p = 0; p < n_passes; p++) {
        mine[(size_t)p * n_pairs] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    RootBox root;
    scene_root(sc, root);
    uint64_t rng = gather_engine(pixel_seed(base_seed, (int32_t)sample, (int32_t)index));
    // the first ray: the caller's as it is -- nothing is drawn --, or the capture's
    V3 pos, d0;
    bool alive = true;
    if(rays != nullptr) {
        const float *r = rays + 6 * (size_t)index;
        pos = v3(r[0], r[1], r[2]);
        d0 = v3(r[3], r[4], r[5]);
    }
    else {
        alive = capture_ray(cap, index, rng, pos, d0);
    }
    LightPassSink sink{{}, groups, n_materials, split != 0u ? 3u : 1u, split, mine, n_pairs};
    sink.flags = alive ? 0u : PT_RADIANCE_OUTSIDE;
    const C4 out = sample_walk<false, true>(tr, sc, root, epsilon, rng, alive, pos, d0, sink);
    plane[gid] = make_float4(out.r, out.g, out.b, __uint_as_float(sink.flags));
}

// The pass records of the rays or pixels first .. first + n - 1 from the chunk's workspace: one wavefront per (ray or pixel, pass), four
// to a workgroup, in pt_radiance_reduce_kernel's order: lane j sums the samples j, j + 64, ... (coalesced), the 64 partials of a
// component are added in lane order by one lane per component, through LDS.  The record goes out as one 16-byte store.
template<int WAVES>
__global__ __launch_bounds__(64 * WAVES) void pt_light_pass_reduce_kernel(const float4 *__restrict__ passes, uint32_t first, uint32_t n, uint32_t samples, uint32_t n_passes,
                                                                          float4 *__restrict__ out) {
    __shared__ float partial[WAVES][3][65];
    __shared__ float4 record[WAVES];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t unit = (size_t)blockIdx.x * WAVES + wave; // (ray or pixel) * n_passes + pass
    const bool there = unit < (size_t)n * n_passes;
    const uint32_t i = there ? (uint32_t)(unit / n_passes) : 0u, p = there ? (uint32_t)(unit - (size_t)i * n_passes) : 0u;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if(there) {
        const float4 *mine = passes + (size_t)p * ((size_t)n * samples) + (size_t)i * samples;
        for(uint32_t s = lane; s < samples; s += 64) {
            const float4 L = mine[s];
            acc[0] = acc[0] + L.x;
            acc[1] = acc[1] + L.y;
            acc[2] = acc[2] + L.z;
        }
    }
    for(int k = 0; k < 3; k++) {
        partial[wave][k][lane] = acc[k];
    }
    __syncthreads();
    float *rec = reinterpret_cast<float *>(&record[wave]);
    if(lane < 3) {
        float sum = 0.0f;
        for(int l = 0; l < 64; l++) {
            sum = sum + partial[wave][lane][l];
        }
        rec[lane] = sum / (float)samples;
    }
    else if(lane == 3) {
        rec[3] = __uint_as_float(0u);
    }
    __syncthreads();
    if(there && lane == 0) {
        out[(size_t)(first + i) * n_passes + p] = record[wave];
    }
}

// out[i] = the mix of the n_passes passes of ray or pixel i under gains[n_passes][3], in the header's order; alpha from total, or 0
__global__ __launch_bounds__(256) void pt_light_pass_mix_kernel(const float4 *__restrict__ passes, size_t n, uint32_t n_passes, const float *__restrict__ gains,
                                                                const float4 *__restrict__ total, float4 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if(i >= n) {
        return;
    }
    float r = 0.0f, g = 0.0f, b = 0.0f;
    const float4 *mine = passes + i * n_passes;
    for(uint32_t p = 0; p < n_passes; p++) {
        const float4 v = mine[p];
        r = r + v.x * gains[3 * p];
        g = g + v.y * gains[3 * p + 1];
        b = b + v.z * gains[3 * p + 2];
    }
    out[i] = make_float4(r, g, b, total != nullptr ? total[2 * i].w : 0.0f);
}

} // namespace

void pt_launch_light_passes(hipStream_t stream, const PtDevScene &scene, const float *rays, const PtCaptureParams &capture, uint32_t first, uint32_t n, uint32_t samples, float epsilon,
                            uint64_t base_seed, const uint8_t *groups, uint32_t n_passes, uint32_t split, float4 *plane, float4 *passes, float4 *out_passes, float4 *out_total,
                            const PtPathConfig &cfg) {
    if(n == 0 || samples == 0 || n_passes == 0) {
        return;
    }
    const uint32_t n_pairs = n * samples;
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        hipLaunchKernelGGL((pt_light_pass_sample_kernel<decltype(window)::value, decltype(in_lds)::value>), dim3((n_pairs + 255) / 256), dim3(256), lds, stream, scene, rays, capture, first,
                           samples, n_pairs, epsilon, base_seed, groups, scene.n_materials, n_passes, split, plane, passes, cfg.spill, cfg.spill_depth);
    });
    const size_t units = (size_t)n * n_passes;
    hipLaunchKernelGGL(pt_light_pass_reduce_kernel<4>, dim3((uint32_t)((units + 3) / 4)), dim3(256), 0, stream, passes, first, n, samples, n_passes, out_passes);
    if(out_total != nullptr) {
        // the total's record is pt_radiance_reduce_kernel's own, from the plane the sampling kernel fills as pt_radiance_sample_kernel does
        hipLaunchKernelGGL(pt_radiance_reduce_kernel<4>, dim3((n + 3) / 4), dim3(256), 0, stream, plane, first, n, samples, out_total);
    }
}

void pt_launch_light_pass_mix(hipStream_t stream, const float4 *passes, size_t n, uint32_t n_passes, const float *gains, const float4 *total, float4 *out) {
    const size_t step = (size_t)1 << 30; // blocks of a launch stay far below 2^31
    for(size_t at = 0; at < n; at += step) {
        const size_t count = n - at < step ? n - at : step;
        hipLaunchKernelGGL(pt_light_pass_mix_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, stream, passes + at * n_passes, count, n_passes, gains,
                           total != nullptr ? total + 2 * at : nullptr, out + at);
    }
}

#endif
