// pt_light_probe_kernels.h -- light probes (include/pt_light_probes.h): the kernel that traces the samples of a chunk of
// probes, the projection that makes their SH records, and the lookup that blends a grid's records at points.  Included by exactly one
// translation unit, pt_walks.hip, behind pt_sample_walk.h and pt_gather_kernels.h, and so behind bind_lane and dispatch_route.
//
// One lane per (probe, sample) pair, sample-fastest, as in pt_gather_kernel, with the engine RandomEngine(pt_pixel_seed(base_seed,
// sample, probe)) -- the PROBE's index in the call.  The sample is the shared loop's (sample_walk, pt_sample_walk.h); what this kernel adds
// to it is the first ray -- (P, d) with d uniform on the sphere, drawn with the sample's first two numbers -- and a sink that keeps two
// flags: the first walk missed, and the first vertex faces away from the ray that reached it.
#ifndef PT_LIGHT_PROBE_KERNELS_H
#define PT_LIGHT_PROBE_KERNELS_H

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_shading.h"

namespace {

using namespace ptd;

// The nine basis functions at d, in the header's association
PT_D void light_probe_basis(float x, float y, float z, float Y[9]) {
    Y[0] = 0.282095f;
    Y[1] = 0.488603f * y;
    Y[2] = 0.488603f * z;
    Y[3] = 0.488603f * x;
    Y[4] = (1.092548f * x) * y;
    Y[5] = (1.092548f * y) * z;
    Y[6] = 0.315392f * ((3.0f * (z * z)) - 1.0f);
    Y[7] = (1.092548f * x) * z;
    Y[8] = 0.546274f * ((x * x) - (y * y));
}

// The flags of a sample: bit 0 missed, bit 1 backfacing (never both: a sample that missed has no first vertex)
struct LightProbeSink : SampleSink {
    uint32_t flags = 0;
    PT_D void first_miss() { flags = 1u; }
    PT_D void first_vertex(V3 n, V3 rd) {
        if(dot(n, rd) > 0.0f) {
            flags = 2u;
        }
    }
};

// The samples of the probes first .. first + n_pairs / samples - 1: plane[2 * g] = L_s, plane[2 * g + 1] = (d, flags: bit 0 missed, bit 1
// backfacing).  positions == null: the probes are the grid's, probe (ix, iy, iz) at origin + (float)i * step.
template<int STACK_LDS, bool IN_LDS>
__global__ __launch_bounds__(256) void pt_light_probe_sample_kernel(PtDevScene sc, const float *__restrict__ positions, PtLightProbeGrid grid, uint32_t first, uint32_t samples,
                                                                    uint32_t n_pairs, float epsilon, uint64_t base_seed, float4 *__restrict__ plane, uint2 *__restrict__ spill,
                                                                    uint32_t spill_depth) {
    Tracer<STACK_LDS, IN_LDS> tr;
    const size_t gid = bind_lane(tr, sc, spill, spill_depth);
    if(gid >= n_pairs) {
        return;
    }
    const uint32_t local = (uint32_t)gid / samples;
    const uint32_t sample = (uint32_t)gid - local * samples;
    const uint32_t probe = first + local;
    RootBox root;
    scene_root(sc, root);
    uint64_t rng = gather_engine(pixel_seed(base_seed, (int32_t)sample, (int32_t)probe));
    V3 pos;
    if(positions != nullptr) {
        const float *p = positions + 3 * (size_t)probe;
        pos = v3(p[0], p[1], p[2]);
    }
    else {
        const uint32_t ix = probe % grid.count[0], rest = probe / grid.count[0];
        const uint32_t iy = rest % grid.count[1], iz = rest / grid.count[1];
        pos = v3(grid.origin[0] + (float)ix * grid.step[0], grid.origin[1] + (float)iy * grid.step[1], grid.origin[2] + (float)iz * grid.step[2]);
    }
    // the direction: uniform on the sphere
    const float u1 = rng_uniform01(rng);
    const float u2 = rng_uniform01(rng);
    const float z = 1.0f - 2.0f * u1;
    const float r = __builtin_sqrtf(1.0f - z * z);
    const float phi = 2.0f * PT_PI_F * u2;
    float sn, cs;
    ptm::sincosf_glibc(phi, &sn, &cs);
    const V3 d0 = v3(r * cs, r * sn, z);

    LightProbeSink sink;
    const C4 out = sample_walk<false, true>(tr, sc, root, epsilon, rng, true, pos, d0, sink);
    plane[2 * gid] = make_float4(out.r, out.g, out.b, 1.0f);
    plane[2 * gid + 1] = make_float4(d0.x, d0.y, d0.z, __uint_as_float(sink.flags));
}

// The records of the probes first .. first + n - 1 from the chunk's workspace: one wavefront per probe, four to a workgroup.  Lane j sums
// its 27 terms over the samples j, j + 64, ... (coalesced: the lanes of a round read neighbouring pairs); the 64 partials of a
// component are added in lane order by one lane per component, through LDS; the counts are sums of ballots.  The record goes out as
// eight 16-byte stores.  (A template, as the lookup below, so that both are emitted behind every instantiation that was there before them
// and no existing kernel's distance to the constant tables changes.)
template<int WAVES>
__global__ __launch_bounds__(64 * WAVES) void pt_light_probe_project_kernel(const float4 *__restrict__ plane, uint32_t first, uint32_t n, uint32_t samples, float4 *__restrict__ out) {
    __shared__ float partial[WAVES][27][65]; // (65: the lanes that add component k's partials read 27 different banks)
    __shared__ float4 record[WAVES][8];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * (uint32_t)WAVES + wave;
    const bool there = i < n;
    float acc[27];
    for(int k = 0; k < 27; k++) {
        acc[k] = 0.0f;
    }
    uint32_t missed = 0, backfacing = 0;
    if(there) {
        const float4 *mine = plane + 2 * ((size_t)i * samples);
        for(uint32_t s0 = 0; s0 < samples; s0 += 64) {
            const uint32_t s = s0 + lane;
            uint32_t flags = 0;
            if(s < samples) {
                const float4 L = mine[2 * (size_t)s];
                const float4 d = mine[2 * (size_t)s + 1];
                flags = __float_as_uint(d.w);
                float Y[9];
                light_probe_basis(d.x, d.y, d.z, Y);
                for(int k = 0; k < 9; k++) {
                    acc[3 * k + 0] = acc[3 * k + 0] + Y[k] * L.x;
                    acc[3 * k + 1] = acc[3 * k + 1] + Y[k] * L.y;
                    acc[3 * k + 2] = acc[3 * k + 2] + Y[k] * L.z;
                }
            }
            missed += (uint32_t)__popcll(__ballot((flags & 1u) != 0));
            backfacing += (uint32_t)__popcll(__ballot((flags & 2u) != 0));
        }
    }
    for(int k = 0; k < 27; k++) {
        partial[wave][k][lane] = acc[k];
    }
    __syncthreads();
    float *rec = reinterpret_cast<float *>(record[wave]);
    if(lane < 27) {
        float sum = 0.0f;
        for(int l = 0; l < 64; l++) {
            sum = sum + partial[wave][lane][l];
        }
        rec[lane] = (sum * (4.0f * PT_PI_F)) / (float)samples;
    }
    else if(lane < 32) {
        rec[lane] = __uint_as_float(lane == 27 ? samples : lane == 28 ? missed : lane == 29 ? backfacing : 0u);
    }
    __syncthreads();
    if(there && lane < 8) {
        out[8 * (size_t)(first + i) + lane] = record[wave][lane];
    }
}

// The lookup: one thread per point blends the eight records around it and evaluates the clamped-cosine convolution towards its normal
template<int BLOCK>
__global__ __launch_bounds__(BLOCK) void pt_light_probe_shade_kernel(PtLightProbeGrid grid, const float4 *__restrict__ probes, float max_backfacing, const float *__restrict__ points6,
                                                                   uint32_t n, float4 *__restrict__ out) {
    const uint32_t t = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
    if(t >= n) {
        return;
    }
    const float *pt = points6 + 6 * (size_t)t;
    int32_t cell[3];
    float f[3];
    for(int a = 0; a < 3; a++) {
        float g = (pt[a] - grid.origin[a]) / grid.step[a];
        g = fminf(fmaxf(g, 0.0f), (float)(grid.count[a] - 1u));
        const float cell_f = floorf(g);
        int32_t i = cell_f >= 2147483648.0f ? 0x7fffffff : (int32_t)cell_f; // ((float)(count - 1) rounds up to 2^31 for counts next to it)
        const int32_t top = (int32_t)grid.count[a] - 2;
        i = i < top ? i : top;
        if(grid.count[a] == 1u) {
            i = 0;
        }
        cell[a] = i;
        f[a] = g - (float)i;
    }
    float b[27];
    for(int k = 0; k < 27; k++) {
        b[k] = 0.0f;
    }
    float wsum = 0.0f;
#pragma unroll 1
    for(int c = 0; c < 8; c++) {
        const int up[3] = {c & 1, (c >> 1) & 1, c >> 2};
        bool exists = true;
        size_t at[3];
        float w3[3];
        for(int a = 0; a < 3; a++) {
            const bool here = !(up[a] != 0 && grid.count[a] == 1u);
            exists = exists && here;
            at[a] = (size_t)cell[a] + (here ? (size_t)up[a] : 0);
            w3[a] = up[a] != 0 ? f[a] : 1.0f - f[a];
        }
        const float4 *p = probes + 8 * ((at[2] * grid.count[1] + at[1]) * grid.count[0] + at[0]);
        float4 q[8];
        for(int k = 0; k < 8; k++) {
            q[k] = p[k];
        }
        const float *rec = reinterpret_cast<const float *>(q);
        const uint32_t taken = __float_as_uint(rec[27]), behind = __float_as_uint(rec[29]);
        float w = (w3[0] * w3[1]) * w3[2];
        if(!exists || (float)behind > max_backfacing * (float)taken) {
            w = 0.0f;
        }
        wsum = wsum + w;
        for(int k = 0; k < 27; k++) {
            b[k] = b[k] + w * rec[k];
        }
    }
    if(wsum == 0.0f) {
        out[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float Y[9];
    light_probe_basis(pt[3], pt[4], pt[5], Y);
    const float a[9] = {1.0f, 2.0f / 3.0f, 2.0f / 3.0f, 2.0f / 3.0f, 0.25f, 0.25f, 0.25f, 0.25f, 0.25f};
    float v[3] = {0.0f, 0.0f, 0.0f};
    for(int k = 0; k < 9; k++) {
        const float ay = a[k] * Y[k];
        for(int c = 0; c < 3; c++) {
            v[c] = v[c] + ay * (b[3 * k + c] / wsum);
        }
    }
    out[t] = make_float4(fmaxf(v[0], 0.0f), fmaxf(v[1], 0.0f), fmaxf(v[2], 0.0f), wsum);
}

} // namespace

void pt_launch_light_probes(hipStream_t stream, const PtDevScene &scene, const float *positions, const PtLightProbeGrid &grid, uint32_t first, uint32_t n_probes, uint32_t samples,
                            float epsilon, uint64_t base_seed, float4 *plane, float4 *out, const PtPathConfig &cfg) {
    if(n_probes == 0 || samples == 0) {
        return;
    }
    const uint32_t n_pairs = n_probes * samples;
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        hipLaunchKernelGGL((pt_light_probe_sample_kernel<decltype(window)::value, decltype(in_lds)::value>), dim3((n_pairs + 255) / 256), dim3(256), lds, stream, scene, positions, grid,
                           first, samples, n_pairs, epsilon, base_seed, plane, cfg.spill, cfg.spill_depth);
    });
    hipLaunchKernelGGL(pt_light_probe_project_kernel<4>, dim3((n_probes + 3) / 4), dim3(256), 0, stream, plane, first, n_probes, samples, out);
}

void pt_launch_light_probe_shade(hipStream_t stream, const PtLightProbeGrid &grid, const float4 *probes, float max_backfacing, const float *points6, uint32_t n, float4 *out) {
    if(n == 0) {
        return;
    }
    hipLaunchKernelGGL(pt_light_probe_shade_kernel<256>, dim3((n + 255) / 256), dim3(256), 0, stream, grid, probes, max_backfacing, points6, n, out);
}

#endif
