// pt_radiance_kernels.h -- radiance along free rays and captures (include/pt_radiance.h): the kernel that traces the samples
// of a chunk of rays or pixels and the reduction that makes their records.  Included by exactly one translation unit, pt_walks.hip, behind
// pt_sample_walk.h and pt_light_probe_kernels.h, and so behind bind_lane and dispatch_route.
//
// One lane per (ray or pixel, sample) pair, sample-fastest, with the engine RandomEngine(pt_pixel_seed(base_seed, sample, index)) -- the
// ray's index in the call, or py * width + px.  The sample is the shared loop's (sample_walk, pt_sample_walk.h); what this kernel adds to
// it is the first ray -- the caller's, or the capture generator's -- and a sink that keeps the flags of the sample's alpha, which leave
// the lane with L_s in one float4.  A sample without a ray (FISHEYE outside the image circle) starts dead and never reaches a walk.
#ifndef PT_RADIANCE_KERNELS_H
#define PT_RADIANCE_KERNELS_H

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_shading.h"

namespace {

using namespace ptd;

#define PT_RADIANCE_MISSED 1u
#define PT_RADIANCE_OUTSIDE 2u

// d[k] = ((right[k] * lx) + (up[k] * ly)) + (forward[k] * lz)
PT_D V3 capture_world(const PtCaptureParams &cap, float lx, float ly, float lz) {
    return v3(((cap.right[0] * lx) + (cap.up[0] * ly)) + (cap.forward[0] * lz), ((cap.right[1] * lx) + (cap.up[1] * ly)) + (cap.forward[1] * lz),
              ((cap.right[2] * lx) + (cap.up[2] * ly)) + (cap.forward[2] * lz));
}

// The ray of a pixel's sample, in the header's order; false: the sample has no ray.  Draws the jitter and nothing else.
PT_D bool capture_ray(const PtCaptureParams &cap, uint32_t pixel, uint64_t &rng, V3 &o, V3 &d) {
    const uint32_t width = (uint32_t)cap.width;
    const uint32_t py = pixel / width, px = pixel - py * width;
    float u1 = 0.5f, u2 = 0.5f;
    if(cap.jitter != 0) {
        u1 = rng_uniform01(rng);
        u2 = rng_uniform01(rng);
    }
    o = v3(cap.origin[0], cap.origin[1], cap.origin[2]);
    if(cap.model == PT_CAPTURE_MODEL_CUBE) {
        const uint32_t N = (uint32_t)cap.height, k = px / N;
        const float a = 2.0f * (((float)(px - k * N) + u1) / (float)N) - 1.0f;
        const float b = 1.0f - 2.0f * (((float)py + u2) / (float)N);
        float lx, ly, lz;
        switch(k) {
        case 0: lx = 1.0f, ly = b, lz = -a; break;
        case 1: lx = -1.0f, ly = b, lz = a; break;
        case 2: lx = a, ly = 1.0f, lz = -b; break;
        case 3: lx = a, ly = -1.0f, lz = b; break;
        case 4: lx = a, ly = b, lz = 1.0f; break;
        default: lx = -a, ly = b, lz = -1.0f; break;
        }
        d = normalize(capture_world(cap, lx, ly, lz));
        return true;
    }
    const float sx = ((float)px + u1) / (float)width;
    const float sy = ((float)py + u2) / (float)cap.height;
    const float a = 2.0f * sx - 1.0f;
    const float b = 1.0f - 2.0f * sy;
    if(cap.model == PT_CAPTURE_MODEL_EQUIRECT) {
        const float phi = (2.0f * PT_PI_F) * (sx - 0.5f);
        const float theta = PT_PI_F * sy;
        float sp, cp, st, ct;
        ptm::sincosf_glibc(phi, &sp, &cp);
        ptm::sincosf_glibc(theta, &st, &ct);
        d = capture_world(cap, st * sp, ct, st * cp);
        return true;
    }
    if(cap.model == PT_CAPTURE_MODEL_FISHEYE) {
        const float rr = __builtin_sqrtf(a * a + b * b);
        if(rr > 1.0f) {
            d = v3(0.0f, 0.0f, 0.0f);
            return false;
        }
        const float theta = rr * (0.5f * cap.fov);
        float st, ct;
        ptm::sincosf_glibc(theta, &st, &ct);
        if(rr == 0.0f) {
            d = capture_world(cap, 0.0f, 0.0f, 1.0f);
        }
        else {
            d = capture_world(cap, (st * a) / rr, (st * b) / rr, ct);
        }
        return true;
    }
    // ORTHO
    const float ax = a * cap.extent[0], by = b * cap.extent[1];
    o = v3((cap.origin[0] + cap.right[0] * ax) + cap.up[0] * by, (cap.origin[1] + cap.right[1] * ax) + cap.up[1] * by, (cap.origin[2] + cap.right[2] * ax) + cap.up[2] * by);
    d = v3(cap.forward[0], cap.forward[1], cap.forward[2]);
    return true;
}

// The flags of a sample's alpha: 0 the first walk hit, PT_RADIANCE_MISSED, or PT_RADIANCE_OUTSIDE, which the kernel sets where there is no ray
struct RadianceSink : SampleSink {
    uint32_t flags = 0;
    PT_D void first_miss() { flags = PT_RADIANCE_MISSED; }
};

// The samples of the rays or pixels first .. first + n_pairs / samples - 1: plane[g] = (L_s rgb, flags: 0 the first walk hit -- alpha 1 --,
// PT_RADIANCE_MISSED, PT_RADIANCE_OUTSIDE -- alpha 0).  rays == null: the rays are the capture's.
template<int STACK_LDS, bool IN_LDS>
__global__ __launch_bounds__(256) void pt_radiance_sample_kernel(PtDevScene sc, const float *__restrict__ rays, PtCaptureParams cap, uint32_t first, uint32_t samples, uint32_t n_pairs,
                                                                 float epsilon, uint64_t base_seed, float4 *__restrict__ plane, uint2 *__restrict__ spill, uint32_t spill_depth) {
    Tracer<STACK_LDS, IN_LDS> tr;
    const size_t gid = bind_lane(tr, sc, spill, spill_depth);
    if(gid >= n_pairs) {
        return;
    }
    const uint32_t local = (uint32_t)gid / samples;
    const uint32_t sample = (uint32_t)gid - local * samples;
    const uint32_t index = first + local;
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
    RadianceSink sink;
    sink.flags = alive ? 0u : PT_RADIANCE_OUTSIDE;
    const C4 out = sample_walk<false, true>(tr, sc, root, epsilon, rng, alive, pos, d0, sink);
    plane[gid] = make_float4(out.r, out.g, out.b, __uint_as_float(sink.flags));
}

// The records of the rays or pixels first .. first + n - 1 from the chunk's workspace: one wavefront each, four to a workgroup.  Lane j
// sums the samples j, j + 64, ... (coalesced: the lanes of a round read neighbouring pairs); the 64 partials of a component are added in
// lane order by one lane per component, through LDS; the counts are popcounts of ballots.  The record goes out as two 16-byte stores.  (A
// template, as 4.20's two small kernels, so that it is emitted behind every instantiation that was there before it.)
template<int WAVES>
__global__ __launch_bounds__(64 * WAVES) void pt_radiance_reduce_kernel(const float4 *__restrict__ plane, uint32_t first, uint32_t n, uint32_t samples, float4 *__restrict__ out) {
    __shared__ float partial[WAVES][4][65];
    __shared__ float4 record[WAVES][2];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * (uint32_t)WAVES + wave;
    const bool there = i < n;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t missed = 0, outside = 0;
    if(there) {
        const float4 *mine = plane + (size_t)i * samples;
        for(uint32_t s0 = 0; s0 < samples; s0 += 64) {
            const uint32_t s = s0 + lane;
            uint32_t flags = 0;
            if(s < samples) {
                const float4 L = mine[s];
                flags = __float_as_uint(L.w);
                acc[0] = acc[0] + L.x;
                acc[1] = acc[1] + L.y;
                acc[2] = acc[2] + L.z;
                acc[3] = acc[3] + (flags == 0u ? 1.0f : 0.0f);
            }
            missed += (uint32_t)__popcll(__ballot(flags == PT_RADIANCE_MISSED));
            outside += (uint32_t)__popcll(__ballot(flags == PT_RADIANCE_OUTSIDE));
        }
    }
    for(int k = 0; k < 4; k++) {
        partial[wave][k][lane] = acc[k];
    }
    __syncthreads();
    float *rec = reinterpret_cast<float *>(record[wave]);
    if(lane < 4) {
        float sum = 0.0f;
        for(int l = 0; l < 64; l++) {
            sum = sum + partial[wave][lane][l];
        }
        rec[lane] = sum / (float)samples;
    }
    else if(lane < 8) {
        rec[lane] = __uint_as_float(lane == 4 ? samples : lane == 5 ? missed : lane == 6 ? outside : 0u);
    }
    __syncthreads();
    if(there && lane < 2) {
        out[2 * (size_t)(first + i) + lane] = record[wave][lane];
    }
}

} // namespace

void pt_launch_radiance(hipStream_t stream, const PtDevScene &scene, const float *rays, const PtCaptureParams &capture, uint32_t first, uint32_t n, uint32_t samples, float epsilon,
                        uint64_t base_seed, float4 *plane, float4 *out, const PtPathConfig &cfg) {
    if(n == 0 || samples == 0) {
        return;
    }
    const uint32_t n_pairs = n * samples;
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        hipLaunchKernelGGL((pt_radiance_sample_kernel<decltype(window)::value, decltype(in_lds)::value>), dim3((n_pairs + 255) / 256), dim3(256), lds, stream, scene, rays, capture, first,
                           samples, n_pairs, epsilon, base_seed, plane, cfg.spill, cfg.spill_depth);
    });
    hipLaunchKernelGGL(pt_radiance_reduce_kernel<4>, dim3((n + 3) / 4), dim3(256), 0, stream, plane, first, n, samples, out);
}

#endif
