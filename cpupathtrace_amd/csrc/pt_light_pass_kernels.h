// pt_light_pass_kernels.h -- light-group passes (include/pt_light_passes.h): the kernel that traces the samples of a chunk
// of rays or pixels and keeps an accumulator per pass beside the ordinary one, the reduction that makes the pass records, and the mix.
// Included by exactly one translation unit, pt_walks.hip, behind pt_radiance_kernels.h, and so behind capture_ray, gather_engine,
// bind_lane and dispatch_route.
//
// The loop is pt_radiance_sample_kernel's, copied so that no existing kernel changes (4.20 and 4.21 copied theirs for the same reason),
// with one more thing at each of its three addition sites: the term also goes to the lane's cell of one pass.  The accumulators live in
// the chunk's workspace, pass-major -- passes[p * n_pairs + pair], 16 bytes each --, not in registers: 24 passes would be 72 VGPRs on top
// of a loop that already carries the tracer.  The 64 lanes of a wavefront touch 64 neighbouring cells; a lane reads, adds and writes only
// its own cell with plain vector loads and stores, so no atomics are needed, and it zeroes its P cells before its loop.  ONE tr.start /
// tr.step site, as there.
#ifndef PT_LIGHT_PASS_KERNELS_H
#define PT_LIGHT_PASS_KERNELS_H

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_shading.h"

namespace {

using namespace ptd;

// sample_emissive (pt_shading.h) that also hands out the registry index it chose.  The selection -- the first of the sample's three
// numbers, std::lower_bound over the CDF -- is replayed on a COPY of the engine; the sample itself is then sample_emissive's, untouched:
// every draw and every number are its own by construction.
template<typename Tables>
PT_D bool sample_emissive_indexed(const PtDevScene &sc, const Tables &tb, V3 pos, uint64_t &rng, V3 &light_pos, C4 &spectrum, float &pd, uint32_t &object_index) {
    uint64_t peek = rng;
    const float r = rng_uniform01(peek);
    int lo = 0, n = (int)sc.n_emis;
    while(n > 0) {
        const int half = n >> 1;
        if(tb.cdf(lo + half) < r) {
            lo = lo + half + 1;
            n = n - half - 1;
        }
        else {
            n = half;
        }
    }
    object_index = (uint32_t)lo;
    return sample_emissive(sc, tb, pos, rng, light_pos, spectrum, pd);
}

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
    const uint32_t per_group = split != 0u ? 3u : 1u;
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
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
    uint32_t flags = alive ? 0u : PT_RADIANCE_OUTSIDE;

    const uint32_t n_light_samples = sc.n_lights + sc.n_object_samples;
    // getSample's state at its top (worker.cpp:37-43)
    float contribution_unweighted = 1.0f;
    double divisor = 1.0, bounce_pd = 1.0;
    C4 spectrum = c4(1.0f, 1.0f, 1.0f, 1.0f);
    C4 out = c4(0.0f, 0.0f, 0.0f, 0.0f);
    int path_length = 0;
    float bounce_probability = 1.0f;
    bool do_bounce = false;
    uint32_t j = 0;
    uint32_t material_index = 0xFFFFFFFFu;
    V3 n = v3(0.0f, 1.0f, 0.0f), rd = d0;
    bool need = true; // the first ray is there
    float4 ro = make_float4(pos.x, pos.y, pos.z, 0.0f), rdv = make_float4(d0.x, d0.y, d0.z, __uint_as_float(0u));
    C4 pending = c4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t pending_pass = 0; // the pass of `pending`
    while(alive) {
        // ---- advance the vertex until it has a ray to trace -------------------------------------------------------------------------------------
        while(alive && !need) {
            if(j < n_light_samples) {
                // worker.cpp:76-103, light sample j
                V3 light_pos;
                C4 light_spectrum;
                float lpd;
                bool valid;
                uint32_t group;
                if(j < sc.n_lights) {
                    const float4 lp = sc.lights[2 * j];
                    light_pos = v3(lp.x, lp.y, lp.z);
                    light_spectrum = c4(sc.lights[2 * j + 1]);
                    lpd = 1.0f;
                    valid = true;
                    group = (uint32_t)groups[n_materials + j];
                }
                else {
                    uint32_t object_index;
                    valid = sample_emissive_indexed(sc, EmisGlobal{sc}, pos, rng, light_pos, light_spectrum, lpd, object_index);
                    group = valid ? material_group(groups, __float_as_uint(sc.emis[4 * (size_t)object_index + 2].w)) : 0u;
                }
                j += 1;
                if(valid) {
                    const Material mat = material_load(sc.materials, material_index);
                    const V3 to_light = light_pos - pos;
                    const V3 light_dir = normalize(to_light);
                    float shading_factor, shadow_ray_pd;
                    const C4 base_spectrum = bsdf_spectrum(mat, rd, light_dir, n, light_spectrum, true, shading_factor, shadow_ray_pd);
                    if(shadow_ray_pd > 0.0f) {
                        const C4 combined = (base_spectrum * shading_factor) * spectrum;
                        const C4 weighed = combined / (float)(divisor * bounce_pd * lpd * shadow_ray_pd);
                        // adding +-0 never changes out_spectrum (which is never -0), so such a sample needs no ray
                        if(!(weighed.r == 0.0f && weighed.g == 0.0f && weighed.b == 0.0f)) {
                            // k = path_length scatterings lie before a light sample
                            const uint32_t pass = group * per_group + (split != 0u ? (uint32_t)(path_length < 2 ? path_length : 2) : 0u);
                            const float threshold = len(to_light) - epsilon;
                            if(threshold <= 0.0f) {
                                out = out + weighed; // light_t < 0 || light_t >= threshold holds for every light_t
                                pass_add(mine + (size_t)pass * n_pairs, weighed);
                            }
                            else {
                                need = true;
                                pending = weighed;
                                pending_pass = pass;
                                const V3 o2 = pos + light_dir * epsilon;
                                ro = make_float4(o2.x, o2.y, o2.z, threshold);
                                rdv = make_float4(light_dir.x, light_dir.y, light_dir.z, __uint_as_float(PT_DEST_SHADOW));
                            }
                        }
                    }
                }
            }
            else if(!do_bounce) {
                alive = false; // worker.cpp:106-109
            }
            else {
                // worker.cpp:110-138
                bounce_pd *= bounce_probability;
                if(bounce_pd <= 1E-20) {
                    alive = false;
                }
                else {
                    const Material mat = material_load(sc.materials, material_index);
                    float ray_factor, ray_pd;
                    const Ray next_ray = bsdf_propagate(mat, rd, pos, n, epsilon, rng, ray_factor, ray_pd);
                    divisor *= ray_pd;
                    divisor /= ray_factor;
                    contribution_unweighted *= ray_factor;
                    float shading_factor, shading_pd;
                    const C4 shaded = bsdf_spectrum(mat, rd, next_ray.d, n, spectrum, false, shading_factor, shading_pd);
                    divisor *= shading_pd;
                    divisor /= shading_factor;
                    contribution_unweighted *= shading_factor;
                    spectrum = shaded;
                    if(divisor <= 1E-20) {
                        alive = false;
                    }
                    else {
                        need = true;
                        ro = make_float4(next_ray.o.x, next_ray.o.y, next_ray.o.z, 0.0f);
                        rdv = make_float4(next_ray.d.x, next_ray.d.y, next_ray.d.z, __uint_as_float(0u));
                    }
                }
            }
        }
        if(!alive) {
            break;
        }
        // ---- the walk: the first ray's, a shadow ray's or a bounce's --------------------------------------------------------------------------
        Walk w;
        typename Tracer<STACK_LDS, IN_LDS>::Rec rec;
        rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
        tr.start(w, rec, root, ro, rdv);
        uint32_t n_nodes = 0, n_leaves = 0;
        while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
        }
        need = false;
        if(w.dest & PT_DEST_SHADOW) {
            if(!w.occluded) {
                out = out + pending; // worker.cpp:100
                pass_add(mine + (size_t)pending_pass * n_pairs, pending);
            }
        }
        else if(w.best_ref == PT_REF_NONE) {
            alive = false; // worker.cpp:47-49
            if(path_length == 0) {
                flags = PT_RADIANCE_MISSED;
            }
        }
        else {
            // the next vertex, up to the roulette draw (worker.cpp:50-70)
            path_length++;
            rd = v3(rdv.x, rdv.y, rdv.z);
            pos = v3(ro.x, ro.y, ro.z) + rd * w.best_t;
            n = object_normal(sc, w.best_ref, pos, material_index);
            const Material mat = material_load(sc.materials, material_index);
            const C4 emitted = (spectrum * mat.emission) / (float)(divisor * bounce_pd);
            out = out + emitted;
            // k = path_length - 1 scatterings lie before the emission of this vertex
            pass_add(mine + (size_t)(material_group(groups, material_index) * per_group + (split != 0u ? (uint32_t)(path_length < 3 ? path_length - 1 : 2) : 0u)) * n_pairs, emitted);
            bounce_probability = path_length <= 4 ? 1.0f : 0.1f + 0.1f * fmin_std(contribution_unweighted * get_contribution(spectrum), 1.0f);
            do_bounce = rng_uniform01(rng) < bounce_probability;
            j = 0;
        }
    }
    plane[gid] = make_float4(out.r, out.g, out.b, __uint_as_float(flags));
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
