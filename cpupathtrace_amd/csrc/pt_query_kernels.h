// pt_query_kernels.h -- scene queries (include/pt_query.h): the hit record of a walk's result, and the three kernels that
// make it for rays, for pixels and for segments.  Included by exactly one translation unit, pt_walks.hip, behind bind_lane and
// dispatch_route, which the kernels and their launches use; tests/hip/query_probe.hip compiles query_record alone for the host
// (PT_QUERY_RECORD_ONLY).
//
// The walk is pt_closest_kernel's, statement for statement, so t and the reference are its bits; the record is made after it, when the
// walk's registers are dead.  pt_occluded_kernel is the shadow walk the path kernel traces for its light samples (Tracer::begin and
// slow_step: PT_DEST_SHADOW in the destination word, the threshold in the origin's w): it ends at the first leaf hit below the threshold
// and is not pruned there, so `occluded` is exactly "the closest hit lies in [0, t_max)".
#ifndef PT_QUERY_KERNELS_H
#define PT_QUERY_KERNELS_H

#include "pt_device.h"
#include "pt_kernels.h"

namespace ptd {

// The instance and the face of object `obj`.  The instance: the last one whose first object is not above obj, if its range holds obj
// (pt_motion_kernel's search); the face: the triangle's index inside an instance that kept every face, else the face table's word, else
// none.  Both stay 0xffffffff where there is none.  (Shared with pt_nearest_kernels.h: one search, two records.)
PT_D void query_instance_face(const PtQueryTables &qt, uint32_t obj, uint32_t &instance, uint32_t &face) {
    instance = 0xffffffffu;
    face = 0xffffffffu;
    if(qt.n_inst != 0) {
        uint32_t lo = 0, hi = qt.n_inst;
        while(hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if(qt.inst[mid].first <= obj) {
                lo = mid;
            }
            else {
                hi = mid;
            }
        }
        const PtQueryInstance qi = qt.inst[lo];
        if(obj >= qi.first && obj - qi.first < qi.count) {
            instance = qi.instance;
            if(qi.count == qi.n_faces) {
                face = obj - qi.first;
            }
            else if(qt.face_of != nullptr) {
                face = qt.face_of[obj - qt.first_object] - qi.face_first;
            }
        }
    }
}

// The record of one walk: (best_ref, best_t) of the ray (o, d) in scene `sc`, with the instance table and the face table of `qt`.
// r[k] is the record's k-th 16 bytes (include/pt_query.h: pt_hit).  The loads of a triangle are object_normal's own (one 128-byte line).
PT_D void query_record(const PtDevScene &sc, const PtQueryTables &qt, uint32_t best_ref, float best_t, V3 o, V3 d, float4 r[4]) {
    if(best_ref == PT_REF_NONE) {
        r[0] = make_float4(-1.0f, __uint_as_float(0xffffffffu), __uint_as_float(0xffffffffu), __uint_as_float(0xffffffffu)); // t, object -1, instance -1, no face
        r[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));                                                    // PT_NO_MATERIAL
        r[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        r[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float t = best_t;
    const V3 pos = o + d * t;
    uint32_t material;
    const V3 n = object_normal(sc, best_ref, pos, material);
    if(best_ref & PT_REF_SPHERE) {
        const uint32_t obj = sc.sph_meta[(best_ref & PT_REF_INDEX) - (sc.n_tris + 1u)].y;
        r[0] = make_float4(t, __uint_as_float(obj), __uint_as_float(0xffffffffu), __uint_as_float(0xffffffffu));
        r[1] = make_float4(pos.x, pos.y, pos.z, __uint_as_float(material));
        r[2] = make_float4(n.x, n.y, n.z, 0.0f);
        r[3] = make_float4(n.x, n.y, n.z, 0.0f);
        return;
    }
    const float4 *rec = sc.tri_shade + 8 * (size_t)(best_ref & PT_REF_INDEX);
    const TriRec tri = tri_unpack(rec[0], rec[1], rec[2]);
    const uint32_t obj = tri.obj_cull & 0x7fffffffu;
    // tri_normal's barycentrics (include/pt_motion_shapes.h states them)
    const V3 ap = pos - tri.a;
    const float d00 = dot(tri.ab, tri.ab);
    const float d01 = dot(tri.ab, tri.ac);
    const float d11 = dot(tri.ac, tri.ac);
    const float d20 = dot(ap, tri.ab);
    const float d21 = dot(ap, tri.ac);
    const float inv_d = 1.0f / (d00 * d11 - d01 * d01);
    const float b1 = (d11 * d20 - d01 * d21) * inv_d;
    const float b2 = (d00 * d21 - d01 * d20) * inv_d;
    const V3 c = cross(tri.ab, tri.ac);
    const float l = (c.x * c.x + c.y * c.y) + c.z * c.z;
    const float inv_l = 1.0f / __builtin_sqrtf(l);
    const bool flat = !(l > 0.0f);
    const V3 g = v3(flat ? 0.0f : c.x * inv_l, flat ? 0.0f : c.y * inv_l, flat ? 0.0f : c.z * inv_l);
    uint32_t instance, face;
    query_instance_face(qt, obj, instance, face);
    r[0] = make_float4(t, __uint_as_float(obj), __uint_as_float(instance), __uint_as_float(face));
    r[1] = make_float4(pos.x, pos.y, pos.z, __uint_as_float(material));
    r[2] = make_float4(n.x, n.y, n.z, b1);
    r[3] = make_float4(g.x, g.y, g.z, b2);
}

} // namespace ptd

#ifndef PT_QUERY_RECORD_ONLY

namespace {

using namespace ptd;

// pt_closest_kernel's walk of the ray (o, d), then its record, stored as four 16-byte vectors
template<int STACK_LDS, bool IN_LDS>
PT_D void query_walk(const Tracer<STACK_LDS, IN_LDS> &tr, const PtDevScene &sc, const PtQueryTables &qt, V3 o, V3 d, float4 *__restrict__ out) {
    Walk w;
    typename Tracer<STACK_LDS, IN_LDS>::Rec rec;
    rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    tr.start(w, rec, root, make_float4(o.x, o.y, o.z, 0.0f), make_float4(d.x, d.y, d.z, __uint_as_float(0u)));
    uint32_t n_nodes = 0, n_leaves = 0;
    while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
    }
    float4 r[4];
    query_record(sc, qt, w.best_ref, w.best_t, o, d, r);
    out[0] = r[0];
    out[1] = r[1];
    out[2] = r[2];
    out[3] = r[3];
}

// pt_query_rays: one ray per lane
template<int STACK_LDS, bool IN_LDS>
__global__ __launch_bounds__(256) void pt_query_kernel(PtDevScene sc, const float *__restrict__ rays6, uint32_t n, float4 *__restrict__ out, uint2 *__restrict__ spill,
                                                       uint32_t spill_depth, PtQueryTables qt) {
    Tracer<STACK_LDS, IN_LDS> tr;
    const size_t gid = bind_lane(tr, sc, spill, spill_depth);
    if(gid >= n) {
        return;
    }
    const float *r = rays6 + 6 * gid;
    query_walk(tr, sc, qt, v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]), out + 4 * gid);
}

// pt_query_pixels (xy[n][2]) and pt_query_frame (kFrame: lane gid is pixel gid of the width x height frame, n = width * height): the
// feature kernel's camera ray with a sub-pixel offset of 0 -- the centre of the pixel --, aperture none, no jitter
template<int STACK_LDS, bool IN_LDS, bool kFrame>
__global__ __launch_bounds__(256) void pt_query_pixels_kernel(PtDevScene sc, PtDevCamera cam, int32_t width, int32_t height, const int32_t *__restrict__ xy, uint32_t n,
                                                              float4 *__restrict__ out, uint2 *__restrict__ spill, uint32_t spill_depth, PtQueryTables qt) {
    Tracer<STACK_LDS, IN_LDS> tr;
    const size_t gid = bind_lane(tr, sc, spill, spill_depth);
    if(gid >= n) {
        return;
    }
    int32_t px, py;
    if constexpr(kFrame) {
        px = (int32_t)(gid % (size_t)width);
        py = (int32_t)(gid / (size_t)width);
    }
    else {
        px = xy[2 * gid];
        py = xy[2 * gid + 1];
    }
    const float one_half = 1.0f / 2.0f;
    const float x_camera = 2 * (((float)px + one_half) / (float)width - one_half);
    float y_camera = 2 * (((float)py + one_half) / (float)height - one_half);
    y_camera = -y_camera;
    uint64_t rng = 0; // (drawn from, never used: both offsets are +0 and there is no aperture)
    const Ray ray = camera_shoot(cam, x_camera, y_camera, 0.0f, 0.0f, rng);
    query_walk(tr, sc, qt, ray.o, ray.d, out + 4 * gid);
}

// pt_occluded_rays: one segment (o, d, t_max) per lane, as a shadow walk with the threshold t_max
template<int STACK_LDS, bool IN_LDS>
__global__ __launch_bounds__(256) void pt_occluded_kernel(PtDevScene sc, const float *__restrict__ seg7, uint32_t n, uint8_t *__restrict__ out, uint2 *__restrict__ spill,
                                                          uint32_t spill_depth) {
    Tracer<STACK_LDS, IN_LDS> tr;
    const size_t gid = bind_lane(tr, sc, spill, spill_depth);
    if(gid >= n) {
        return;
    }
    const float *r = seg7 + 7 * gid;
    Walk w;
    typename Tracer<STACK_LDS, IN_LDS>::Rec rec;
    rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    tr.start(w, rec, root, make_float4(r[0], r[1], r[2], r[6]), make_float4(r[3], r[4], r[5], __uint_as_float(PT_DEST_SHADOW)));
    uint32_t n_nodes = 0, n_leaves = 0;
    while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
    }
    out[gid] = w.occluded ? 1 : 0;
}

} // namespace

void pt_launch_query_rays(hipStream_t stream, const PtDevScene &scene, const float *rays6, uint32_t n, float4 *out, const PtQueryTables &tables, const PtPathConfig &cfg) {
    if(n == 0) {
        return;
    }
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        hipLaunchKernelGGL((pt_query_kernel<decltype(window)::value, decltype(in_lds)::value>), dim3((n + 255) / 256), dim3(256), lds, stream, scene, rays6, n, out, cfg.spill,
                           cfg.spill_depth, tables);
    });
}

void pt_launch_query_pixels(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, int32_t width, int32_t height, const int32_t *xy, uint32_t n, float4 *out,
                            const PtQueryTables &tables, const PtPathConfig &cfg) {
    if(n == 0 || width <= 0 || height <= 0) {
        return;
    }
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        constexpr int kWindow = decltype(window)::value;
        constexpr bool kInLds = decltype(in_lds)::value;
        if(xy == nullptr) {
            hipLaunchKernelGGL((pt_query_pixels_kernel<kWindow, kInLds, true>), dim3((n + 255) / 256), dim3(256), lds, stream, scene, camera, width, height, xy, n, out,
                               cfg.spill, cfg.spill_depth, tables);
        }
        else {
            hipLaunchKernelGGL((pt_query_pixels_kernel<kWindow, kInLds, false>), dim3((n + 255) / 256), dim3(256), lds, stream, scene, camera, width, height, xy, n, out,
                               cfg.spill, cfg.spill_depth, tables);
        }
    });
}

void pt_launch_occluded(hipStream_t stream, const PtDevScene &scene, const float *seg7, uint32_t n, uint8_t *out, const PtPathConfig &cfg) {
    if(n == 0) {
        return;
    }
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        hipLaunchKernelGGL((pt_occluded_kernel<decltype(window)::value, decltype(in_lds)::value>), dim3((n + 255) / 256), dim3(256), lds, stream, scene, seg7, n, out, cfg.spill,
                           cfg.spill_depth);
    });
}

#endif // PT_QUERY_RECORD_ONLY

#endif
