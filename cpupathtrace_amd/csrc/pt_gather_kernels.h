// pt_gather_kernels.h -- light gathered at surface points (include/pt_gather.h): the kernel that traces the samples of a
// chunk of points, the ordered reduce that makes their records, and the two kernels that make points from a frame's first hits and from
// an instance's triangle records.  Included by exactly one translation unit, pt_walks.hip, behind bind_lane and dispatch_route, behind
// pt_query_kernels.h, whose walk and record the frame's points are made with, and behind pt_sample_walk.h.
//
// One lane per (point, sample) pair, sample-fastest: lane g of a chunk that starts at point p0 is sample g % samples of point p0 +
// g / samples, with the engine RandomEngine(pt_pixel_seed(base_seed, sample, point)) -- the POINT's index in the call, not in the chunk,
// so a value does not depend on how the call is cut.  The direct light and the full paths are the shared loop's (sample_walk,
// pt_sample_walk.h); what this kernel adds to it is the entry: a sample starts at a vertex that is already there, the point with its
// normal and no material, and the direct kind never bounces.  It sets no flag and keeps no term apart, so its sink is the empty one.
// The occlusion kind is not a path sample: one bsdf_propagate at the receiver and one shadow walk of its own.
#ifndef PT_GATHER_KERNELS_H
#define PT_GATHER_KERNELS_H

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_shading.h"

namespace {

using namespace ptd;

// The samples of the points first .. first + n_pairs / samples - 1.  KIND 0 (PT_GATHER_OCCLUSION): bits[g / 64] bit g % 64 = sample g is
// occluded (one 8-byte store per wavefront; the grid's last wavefront writes zeros for the lanes past n_pairs).  KIND 1, 2: plane[g] = the
// sample's out_spectrum.  `miss` (null: none): points that are not there -- a frame's pixels without a first hit --, whose lanes trace nothing.
template<int STACK_LDS, bool IN_LDS, int KIND>
__global__ __launch_bounds__(256) void pt_gather_kernel(PtDevScene sc, const float *__restrict__ points6, const uint8_t *__restrict__ miss, uint32_t first, uint32_t samples,
                                                        uint32_t n_pairs, float epsilon, float distance, uint64_t base_seed, float4 *__restrict__ plane,
                                                        unsigned long long *__restrict__ bits, uint2 *__restrict__ spill, uint32_t spill_depth) {
    Tracer<STACK_LDS, IN_LDS> tr;
    const size_t gid = bind_lane(tr, sc, spill, spill_depth);
    const bool lane_live = gid < n_pairs;
    if constexpr(KIND != 0) {
        if(!lane_live) {
            return;
        }
    }
    const uint32_t local = lane_live ? (uint32_t)gid / samples : 0u;
    const uint32_t sample = lane_live ? (uint32_t)gid - local * samples : 0u;
    const uint32_t point = first + local;
    const bool there = lane_live && (miss == nullptr || miss[point] == 0);
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    uint64_t rng = gather_engine(pixel_seed(base_seed, (int32_t)sample, (int32_t)point));
    const float *pt = points6 + 6 * (size_t)point;
    V3 pos = v3(0.0f, 0.0f, 0.0f), n = v3(0.0f, 1.0f, 0.0f);
    if(there) {
        pos = v3(pt[0], pt[1], pt[2]);
        n = v3(pt[3], pt[4], pt[5]);
    }

    if constexpr(KIND == 0) {
        bool occluded = false;
        if(there) {
            const V3 rd = neg(n);
            const uint32_t material_index = 0xFFFFFFFFu; // PT_NO_MATERIAL: the receiver
            const Material mat = material_load(sc.materials, material_index);
            float ray_factor, ray_pd;
            const Ray next = bsdf_propagate(mat, rd, pos, n, epsilon, rng, ray_factor, ray_pd);
            Walk w;
            typename Tracer<STACK_LDS, IN_LDS>::Rec rec;
            rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
            tr.start(w, rec, root, make_float4(next.o.x, next.o.y, next.o.z, distance), make_float4(next.d.x, next.d.y, next.d.z, __uint_as_float(PT_DEST_SHADOW)));
            uint32_t n_nodes = 0, n_leaves = 0;
            while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
            }
            occluded = w.occluded;
        }
        const unsigned long long word = __ballot(occluded);
        if((threadIdx.x & 63) == 0 && (gid & ~(size_t)63) < n_pairs) {
            bits[gid >> 6] = word;
        }
        return;
    }
    else {
        SampleSink sink;
        const C4 out = sample_walk<true, KIND == 2>(tr, sc, root, epsilon, rng, there, pos, n, sink);
        plane[gid] = there ? make_float4(out.r, out.g, out.b, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// The records of the points first .. first + n - 1 from the chunk's workspace: one thread per point sums its samples in index order
// (fp32, from 0) and divides by (float)samples; out[2 * p], out[2 * p + 1] are the record's two 16-byte halves.  A point that is not
// there gets the all-zero record.
template<int KIND>
__global__ __launch_bounds__(256) void pt_gather_reduce_kernel(const float4 *__restrict__ plane, const unsigned long long *__restrict__ bits, const uint8_t *__restrict__ miss,
                                                               uint32_t first, uint32_t n, uint32_t samples, float4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if(i >= n) {
        return;
    }
    const uint32_t point = first + i;
    float4 *o = out + 2 * (size_t)point;
    if(miss != nullptr && miss[point] != 0) {
        o[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        o[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const size_t base = (size_t)i * samples;
    if constexpr(KIND == 0) {
        uint32_t occluded = 0;
        for(uint32_t s = 0; s < samples; s++) {
            const size_t g = base + s;
            occluded += (uint32_t)((bits[g >> 6] >> (g & 63)) & 1ULL);
        }
        const float v = (float)(samples - occluded) / (float)samples;
        o[0] = make_float4(v, v, v, 1.0f);
        o[1] = make_float4(__uint_as_float(samples), __uint_as_float(occluded), __uint_as_float(0u), __uint_as_float(0u));
    }
    else {
        float r = 0.0f, g = 0.0f, b = 0.0f;
        for(uint32_t s = 0; s < samples; s++) {
            const float4 v = plane[base + s];
            r = r + v.x;
            g = g + v.y;
            b = b + v.z;
        }
        const float d = (float)samples;
        o[0] = make_float4(r / d, g / d, b / d, 1.0f);
        o[1] = make_float4(__uint_as_float(samples), __uint_as_float(0u), __uint_as_float(0u), __uint_as_float(0u));
    }
}

// A frame's points: pt_query_pixels_kernel's ray through the centre of pixel gid and its walk; the point is the hit's position and its
// shading normal, negated where dot(normal, d) > 0; miss[gid] = 1 where the ray hits nothing (the point's six floats are 0 then).
template<int STACK_LDS, bool IN_LDS>
__global__ __launch_bounds__(256) void pt_gather_frame_points_kernel(PtDevScene sc, PtDevCamera cam, int32_t width, int32_t height, uint32_t n, float *__restrict__ points6,
                                                                     uint8_t *__restrict__ miss, uint2 *__restrict__ spill, uint32_t spill_depth) {
    Tracer<STACK_LDS, IN_LDS> tr;
    const size_t gid = bind_lane(tr, sc, spill, spill_depth);
    if(gid >= n) {
        return;
    }
    const int32_t px = (int32_t)(gid % (size_t)width);
    const int32_t py = (int32_t)(gid / (size_t)width);
    const float one_half = 1.0f / 2.0f;
    const float x_camera = 2 * (((float)px + one_half) / (float)width - one_half);
    float y_camera = 2 * (((float)py + one_half) / (float)height - one_half);
    y_camera = -y_camera;
    uint64_t rng = 0; // (drawn from, never used: both offsets are +0 and there is no aperture)
    const Ray ray = camera_shoot(cam, x_camera, y_camera, 0.0f, 0.0f, rng);
    Walk w;
    typename Tracer<STACK_LDS, IN_LDS>::Rec rec;
    rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    tr.start(w, rec, root, make_float4(ray.o.x, ray.o.y, ray.o.z, 0.0f), make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(0u)));
    uint32_t n_nodes = 0, n_leaves = 0;
    while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
    }
    float *p = points6 + 6 * gid;
    if(w.best_ref == PT_REF_NONE) {
        for(int k = 0; k < 6; k++) {
            p[k] = 0.0f;
        }
        miss[gid] = 1;
        return;
    }
    const V3 pos = ray.o + ray.d * w.best_t; // query_record's position
    uint32_t material;
    V3 nrm = object_normal(sc, w.best_ref, pos, material);
    if(dot(nrm, ray.d) > 0.0f) {
        nrm = neg(nrm);
    }
    p[0] = pos.x;
    p[1] = pos.y;
    p[2] = pos.z;
    p[3] = nrm.x;
    p[4] = nrm.y;
    p[5] = nrm.z;
    miss[gid] = 0;
}

// An instance's points: corner c of triangle first_tri + t is point 3 t + c, its position from the kept positions and its normal from the
// shading record (pt_mesh.hip k_unpack: what pt_scene_get_triangles returns as out_pos and out_nrm).
__global__ __launch_bounds__(256) void pt_gather_corner_points_kernel(const float *__restrict__ pos, const float4 *__restrict__ shade, uint32_t first_tri, uint32_t n_tris,
                                                                      float *__restrict__ points6) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if(t >= n_tris) {
        return;
    }
    const size_t tri = (size_t)first_tri + t;
    const float4 *sh = shade + 8 * tri;
    const float4 a = sh[3], b = sh[4], c = sh[5];
    const float q[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x};
    float *o = points6 + 18 * (size_t)t;
    for(int corner = 0; corner < 3; corner++) {
        for(int k = 0; k < 3; k++) {
            o[6 * corner + k] = pos[9 * tri + 3 * corner + k];
            o[6 * corner + 3 + k] = q[3 * corner + k];
        }
    }
}

} // namespace

void pt_launch_gather(hipStream_t stream, const PtDevScene &scene, int kind, const float *points6, const uint8_t *miss, uint32_t first, uint32_t n_points, uint32_t samples,
                      float epsilon, float distance, uint64_t base_seed, float4 *plane, unsigned long long *bits, float4 *out, const PtPathConfig &cfg) {
    if(n_points == 0 || samples == 0) {
        return;
    }
    const uint32_t n_pairs = n_points * samples;
    const dim3 grid((n_pairs + 255) / 256), reduce_grid((n_points + 255) / 256);
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        constexpr int kWindow = decltype(window)::value;
        constexpr bool kInLds = decltype(in_lds)::value;
        if(kind == 0) {
            hipLaunchKernelGGL((pt_gather_kernel<kWindow, kInLds, 0>), grid, dim3(256), lds, stream, scene, points6, miss, first, samples, n_pairs, epsilon, distance, base_seed,
                               plane, bits, cfg.spill, cfg.spill_depth);
        }
        else if(kind == 1) {
            hipLaunchKernelGGL((pt_gather_kernel<kWindow, kInLds, 1>), grid, dim3(256), lds, stream, scene, points6, miss, first, samples, n_pairs, epsilon, distance, base_seed,
                               plane, bits, cfg.spill, cfg.spill_depth);
        }
        else {
            hipLaunchKernelGGL((pt_gather_kernel<kWindow, kInLds, 2>), grid, dim3(256), lds, stream, scene, points6, miss, first, samples, n_pairs, epsilon, distance, base_seed,
                               plane, bits, cfg.spill, cfg.spill_depth);
        }
    });
    if(kind == 0) {
        hipLaunchKernelGGL((pt_gather_reduce_kernel<0>), reduce_grid, dim3(256), 0, stream, plane, bits, miss, first, n_points, samples, out);
    }
    else {
        hipLaunchKernelGGL((pt_gather_reduce_kernel<1>), reduce_grid, dim3(256), 0, stream, plane, bits, miss, first, n_points, samples, out);
    }
}

void pt_launch_gather_frame_points(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, int32_t width, int32_t height, float *points6, uint8_t *miss,
                                   const PtPathConfig &cfg) {
    if(width <= 0 || height <= 0) {
        return;
    }
    const uint32_t n = (uint32_t)width * (uint32_t)height;
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        hipLaunchKernelGGL((pt_gather_frame_points_kernel<decltype(window)::value, decltype(in_lds)::value>), dim3((n + 255) / 256), dim3(256), lds, stream, scene, camera, width,
                           height, n, points6, miss, cfg.spill, cfg.spill_depth);
    });
}

void pt_launch_gather_corner_points(hipStream_t stream, const float *pos, const float4 *shade, uint32_t first_tri, uint32_t n_tris, float *points6) {
    if(n_tris == 0) {
        return;
    }
    hipLaunchKernelGGL(pt_gather_corner_points_kernel, dim3((n_tris + 255) / 256), dim3(256), 0, stream, pos, shade, first_tri, n_tris, points6);
}

#endif
