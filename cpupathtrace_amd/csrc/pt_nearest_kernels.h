// pt_nearest_kernels.h -- nearest-surface queries (include/pt_nearest.h): the closest point of a triangle and of a
// sphere to a free point, the lower bound of a box that orders and prunes the walk, the record of an answer, and the kernel that walks
// the tree for points and for the cells of a grid.  Included by exactly one translation unit of the product, pt_nearest.hip;
// tests/hip/nearest_probe.hip compiles the device functions alone for the host (PT_NEAREST_FUNCTIONS_ONLY).
//
// The answer is DEFINED as a minimum over all objects (include/pt_nearest.h); the walk only skips work, and must skip nothing that
// could be the answer -- or tie with it.
//
// THE PRUNING RULE.  The plain box distance, the sum over the axes of max(lo - p, p - hi, 0)^2, is NOT a lower bound of the computed
// d2 of what the box holds: the closest point comes out of a chain of rounded products, and the computed d2 of a triangle falls below
// the plain distance to that triangle's own box for 1-2 % of random (point, triangle) pairs near the origin, by up to about 2 ulp of M
// in distance, M the largest coordinate magnitude among p and the root box (tests/test_nearest_cpu.py measures it again).  So, with M
// computed once per query:
//     per axis  g = max(max(lo - p, p - hi), 0),  g' = max(g - m, 0)  with  m = M * 2^-18
//     bound = (g'.g') * (1 - 2^-20)
// and a subtree is skipped only when bound > best, STRICTLY: an object at exactly the best distance with a lower record index
// elsewhere is still visited.  `best` is r2 until an object is held.  A loose margin costs time, never the answer; the comparison is
// never tightened.
//
// THE WALK.  One query per lane, 256 lanes per workgroup.  A lane's stack holds (child reference, bits of the child's bound); it has
// Tracer's layout (pt_trace.h): entry e of the top NEAREST_WINDOW entries in LDS at [(e mod W) * 256 + lane], older entries in the
// lane's spill area in HBM.  The walk descends the nearer child and parks the farther one, so it never holds more than one entry per
// level of the tree: the spill area PtPathConfig::spill_depth describes (depth + 2 - window, pt_render.cpp) is deep enough.  A step
// fetches the 64-byte record the walk stands on with four 16-byte loads.  On a pair record it forms both bounds, descends the nearer
// child and parks the farther one unless it is pruned; on a leaf it runs the arithmetic of include/pt_nearest.h and takes the object if
// d2 < best, or d2 == best and its record index is below the holder's, or -- no holder yet -- d2 <= r2.  A pop discards the entries
// whose stored bound prunes by now.
#ifndef PT_NEAREST_KERNELS_H
#define PT_NEAREST_KERNELS_H

#ifndef PT_QUERY_RECORD_ONLY
#define PT_QUERY_RECORD_ONLY // query_instance_face alone: the walks of pt_query_kernels.h stay in pt_walks.hip
#endif
#include "pt_query_kernels.h"

namespace ptd {

#define PT_NEAREST_MARGIN 0x1p-18f        /* m = M * 2^-18 */
#define PT_NEAREST_SHRINK 0x1.ffffep-1f   /* 1 - 2^-20 */

// What one object answers: the squared distance, the weights of the closest point and the feature it lies on
struct NearestHit {
    float d2;
    float v, w;
    uint32_t feature;
};

// include/pt_nearest.h, "Triangle": the closest point of the triangle (a, ab, ac) to p.  diff: p less that point.
PT_D NearestHit nearest_triangle(V3 a, V3 ab, V3 ac, V3 p, V3 &diff) {
    const V3 ap = p - a;
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    const V3 bp = ap - ab;
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    const V3 cp = ap - ac;
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    const float e1 = d4 - d3, e2 = d5 - d6;
    NearestHit h;
    if(d1 <= 0.0f && d2 <= 0.0f) {
        h.v = 0.0f;
        h.w = 0.0f;
        h.feature = 4u;
    }
    else if(d3 >= 0.0f && d4 <= d3) {
        h.v = 1.0f;
        h.w = 0.0f;
        h.feature = 5u;
    }
    else if(vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        h.v = d1 / (d1 - d3);
        h.w = 0.0f;
        h.feature = 1u;
    }
    else if(d6 >= 0.0f && d5 <= d6) {
        h.v = 0.0f;
        h.w = 1.0f;
        h.feature = 6u;
    }
    else if(vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        h.v = 0.0f;
        h.w = d2 / (d2 - d6);
        h.feature = 3u;
    }
    else if(va <= 0.0f && e1 >= 0.0f && e2 >= 0.0f) {
        h.w = e1 / (e1 + e2);
        h.v = 1.0f - h.w;
        h.feature = 2u;
    }
    else {
        const float den = 1.0f / ((va + vb) + vc);
        h.v = vb * den;
        h.w = vc * den;
        h.feature = 0u;
    }
    diff = (ap - ab * h.v) - ac * h.w;
    h.d2 = dot(diff, diff);
    return h;
}

// include/pt_nearest.h, "Sphere": len = |p - c|, dist = |len - R|
PT_D NearestHit nearest_sphere(V3 c, float radius, V3 p, V3 &pc, float &len, float &dist) {
    pc = p - c;
    len = __builtin_sqrtf(dot(pc, pc));
    dist = __builtin_fabsf(len - radius);
    NearestHit h;
    h.d2 = dist * dist;
    h.v = 0.0f;
    h.w = 0.0f;
    h.feature = 7u;
    return h;
}

// The pruning rule's bound of the box (lo, hi) for the point p with the margin m (the header comment)
PT_D float nearest_box_bound(V3 lo, V3 hi, V3 p, float m) {
    const float gx = __builtin_fmaxf(__builtin_fmaxf(lo.x - p.x, p.x - hi.x), 0.0f);
    const float gy = __builtin_fmaxf(__builtin_fmaxf(lo.y - p.y, p.y - hi.y), 0.0f);
    const float gz = __builtin_fmaxf(__builtin_fmaxf(lo.z - p.z, p.z - hi.z), 0.0f);
    const V3 g = v3(__builtin_fmaxf(gx - m, 0.0f), __builtin_fmaxf(gy - m, 0.0f), __builtin_fmaxf(gz - m, 0.0f));
    return dot(g, g) * PT_NEAREST_SHRINK;
}

// m of a query: M * 2^-18, M the largest coordinate magnitude among p and the root box
PT_D float nearest_margin(const float *root_lo, const float *root_hi, V3 p) {
    float big = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(p.x), __builtin_fabsf(p.y)), __builtin_fabsf(p.z));
    for(int k = 0; k < 3; k++) {
        big = __builtin_fmaxf(big, __builtin_fmaxf(__builtin_fabsf(root_lo[k]), __builtin_fabsf(root_hi[k])));
    }
    return big * PT_NEAREST_MARGIN;
}

// Whether the leaf `index` with the squared distance d2 replaces the holder (PT_REF_NONE: none yet, best is r2).  A NaN d2 never does.
PT_D bool nearest_takes(float d2, uint32_t index, float best, uint32_t holder) {
    return holder == PT_REF_NONE ? d2 <= best : (d2 < best) | ((d2 == best) & (index < (holder & PT_REF_INDEX)));
}

PT_D void nearest_miss(float4 r[4]) {
    const float inf = __builtin_inff();
    r[0] = make_float4(inf, __uint_as_float(0xffffffffu), __uint_as_float(0xffffffffu), __uint_as_float(0xffffffffu)); // object -1, instance -1, no face
    r[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));                                                   // PT_NO_MATERIAL
    r[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    r[3] = make_float4(inf, 0.0f, 0.0f, 0.0f);
}

// The record of the answer `holder` (a leaf reference, or PT_REF_NONE: a miss) of the point p: r[k] is the k-th 16 bytes of pt_nearest.
// The leaf's arithmetic is run again on the leaf's record, so every word is the one the walk compared.
PT_D void nearest_record(const PtDevScene &sc, const PtQueryTables &qt, uint32_t holder, V3 p, float4 r[4]) {
    if(holder == PT_REF_NONE) {
        nearest_miss(r);
        return;
    }
    const uint32_t index = holder & PT_REF_INDEX;
    const float4 *rec = sc.recs + 4 * (size_t)index;
    if(holder & PT_REF_SPHERE) {
        const float4 s = rec[0];
        const uint2 meta = sc.sph_meta[index - (sc.n_tris + 1u)];
        const V3 c = v3(s.x, s.y, s.z);
        V3 pc;
        float len, dist;
        const NearestHit h = nearest_sphere(c, s.w, p, pc, len, dist);
        const bool centre = len == 0.0f;
        const V3 on = c + pc * (s.w / len);
        const V3 n = pc * (1.0f / len);
        const int32_t side = len > s.w ? 1 : (len < s.w ? -1 : 0);
        r[0] = make_float4(dist, __uint_as_float(meta.y), __uint_as_float(0xffffffffu), __uint_as_float(0xffffffffu));
        r[1] = make_float4(centre ? c.x + s.w : on.x, centre ? c.y + 0.0f : on.y, centre ? c.z + 0.0f : on.z, __uint_as_float(meta.x));
        r[2] = make_float4(centre ? 1.0f : n.x, centre ? 0.0f : n.y, centre ? 0.0f : n.z, 0.0f);
        r[3] = make_float4(h.d2, __uint_as_float(h.feature), __uint_as_float((uint32_t)side), 0.0f);
        return;
    }
    const TriRec tri = tri_unpack(rec[0], rec[1], rec[2]);
    const uint32_t obj = tri.obj_cull & 0x7fffffffu;
    V3 diff;
    const NearestHit h = nearest_triangle(tri.a, tri.ab, tri.ac, p, diff);
    const V3 pos = (tri.a + tri.ab * h.v) + tri.ac * h.w;
    // pt_hit's geometric normal (query_record)
    const V3 c = cross(tri.ab, tri.ac);
    const float l = (c.x * c.x + c.y * c.y) + c.z * c.z;
    const float inv_l = 1.0f / __builtin_sqrtf(l);
    const bool flat = !(l > 0.0f);
    const V3 g = v3(flat ? 0.0f : c.x * inv_l, flat ? 0.0f : c.y * inv_l, flat ? 0.0f : c.z * inv_l);
    const float s = dot(diff, c);
    const int32_t side = s > 0.0f ? 1 : (s < 0.0f ? -1 : 0);
    uint32_t instance, face;
    query_instance_face(qt, obj, instance, face);
    r[0] = make_float4(__builtin_sqrtf(h.d2), __uint_as_float(obj), __uint_as_float(instance), __uint_as_float(face));
    r[1] = make_float4(pos.x, pos.y, pos.z, __uint_as_float(tri.material));
    r[2] = make_float4(g.x, g.y, g.z, h.v);
    r[3] = make_float4(h.d2, __uint_as_float(h.feature), __uint_as_float((uint32_t)side), h.w);
}

} // namespace ptd

#ifndef PT_NEAREST_FUNCTIONS_ONLY

namespace {

using namespace ptd;

#define PT_NEAREST_WINDOW 8 /* entries of a lane's stack kept in LDS (16 KB per workgroup); deeper ones spill to HBM */

// The walk of the query (p, r): the leaf that answers it, or PT_REF_NONE.  stack_l: the lane's column of the LDS window; my_spill: the
// lane's spill_depth entries in HBM.  visits[0], visits[1]: pair and leaf records fetched.
PT_D uint32_t nearest_walk(const PtDevScene &sc, V3 p, float r, uint2 *stack_l, uint2 *__restrict__ my_spill, uint32_t spill_depth, uint32_t visits[2]) {
    if(!(r >= 0.0f) || p.x != p.x || p.y != p.y || p.z != p.z || sc.root_ref == PT_REF_NONE) {
        return PT_REF_NONE;
    }
    const float m = nearest_margin(sc.root_lo, sc.root_hi, p);
    float best = r * r;
    uint32_t holder = PT_REF_NONE;
    uint32_t cur = sc.root_ref;
    if(nearest_box_bound(ld3(sc.root_lo), ld3(sc.root_hi), p, m) > best) {
        return PT_REF_NONE;
    }
    uint32_t sp = 0;
    const uint32_t room = (uint32_t)PT_NEAREST_WINDOW + spill_depth;
    while(cur != PT_REF_NONE) {
        const float4 *rec = sc.recs + 4 * (size_t)(cur & PT_REF_INDEX);
        const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
        uint32_t next = PT_REF_NONE;
        if(cur & PT_REF_LEAF) {
            visits[1]++;
            float d2;
            if(cur & PT_REF_SPHERE) {
                V3 pc;
                float len, dist;
                d2 = nearest_sphere(v3(q0.x, q0.y, q0.z), q0.w, p, pc, len, dist).d2;
            }
            else {
                const TriRec tri = tri_unpack(q0, q1, q2);
                V3 diff;
                d2 = nearest_triangle(tri.a, tri.ab, tri.ac, p, diff).d2;
            }
            if(nearest_takes(d2, cur & PT_REF_INDEX, best, holder)) {
                best = d2;
                holder = cur;
            }
        }
        else {
            visits[0]++;
            const float bl = nearest_box_bound(v3(q0.x, q0.y, q0.z), v3(q0.w, q1.x, q1.y), p, m);
            const float br = nearest_box_bound(v3(q1.z, q1.w, q2.x), v3(q2.y, q2.z, q2.w), p, m);
            const uint32_t left = __float_as_uint(q3.x), right = __float_as_uint(q3.y);
            const bool go_l = !(bl > best) && left != PT_REF_NONE, go_r = !(br > best) && right != PT_REF_NONE;
            if(go_l && go_r) {
                const bool left_first = bl <= br;
                next = left_first ? left : right;
                // (room is never short: one parked entry per level, and the spill area is as deep as the tree.  The test keeps a
                // tree that breaks that promise from writing outside the lane's area.)
                if(sp < room) {
                    const uint2 far = make_uint2(left_first ? right : left, __float_as_uint(left_first ? br : bl));
                    const uint32_t slot = (sp & (uint32_t)(PT_NEAREST_WINDOW - 1)) * 256u;
                    if(sp >= (uint32_t)PT_NEAREST_WINDOW) {
                        my_spill[sp - PT_NEAREST_WINDOW] = stack_l[slot]; // the window moves up: its oldest entry leaves
                    }
                    stack_l[slot] = far;
                    sp++;
                }
            }
            else if(go_l | go_r) {
                next = go_l ? left : right;
            }
        }
        // a leaf, or a pair with both children pruned: back to the first parked entry whose bound does not prune by now
        while(next == PT_REF_NONE && sp != 0) {
            const uint32_t below = sp - 1u;
            const uint32_t slot = (below & (uint32_t)(PT_NEAREST_WINDOW - 1)) * 256u;
            const uint2 e = stack_l[slot];
            if(below >= (uint32_t)PT_NEAREST_WINDOW) {
                stack_l[slot] = my_spill[below - PT_NEAREST_WINDOW]; // the window moves down: the entry that left it last comes back
            }
            sp = below;
            if(!(__uint_as_float(e.y) > best)) {
                next = e.x;
            }
        }
        cur = next;
    }
    return holder;
}

// kGrid: lane gid is cell first + gid of the grid, the query (origin + i * step, max_distance), and writes distance and object;
// otherwise query first + gid of points4 (xyz, max_distance), and writes its record.  The spill area belongs to the LAUNCH: lane gid has
// entries [gid * spill_depth, (gid + 1) * spill_depth).  counts (diagnostic, may be null): pair and leaf records fetched by the launch.
template<bool kGrid>
__global__ __launch_bounds__(256) void pt_nearest_kernel(PtDevScene sc, PtQueryTables qt, const float *__restrict__ points4, PtDistanceGrid grid, float max_distance,
                                                         uint32_t first, uint32_t n, float4 *__restrict__ out, float *__restrict__ out_distance,
                                                         int32_t *__restrict__ out_object, uint2 *__restrict__ spill, uint32_t spill_depth,
                                                         unsigned long long *__restrict__ counts) {
    __shared__ uint2 stack[PT_NEAREST_WINDOW * 256];
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if(gid >= n) {
        return;
    }
    const size_t item = (size_t)first + gid;
    V3 p;
    float r;
    if constexpr(kGrid) {
        const uint32_t nx = grid.count[0], ny = grid.count[1];
        const uint32_t ix = (uint32_t)(item % nx), iy = (uint32_t)((item / nx) % ny), iz = (uint32_t)(item / ((size_t)nx * ny));
        p = v3(grid.origin[0] + (float)ix * grid.step[0], grid.origin[1] + (float)iy * grid.step[1], grid.origin[2] + (float)iz * grid.step[2]);
        r = max_distance;
    }
    else {
        const float *q = points4 + 4 * item; // (four words, not one vector: the caller's array need not be 16-byte aligned)
        p = v3(q[0], q[1], q[2]);
        r = q[3];
    }
    uint32_t visits[2] = {0u, 0u};
    const uint32_t holder = nearest_walk(sc, p, r, stack + threadIdx.x, spill + (size_t)gid * spill_depth, spill_depth, visits);
    float4 rec[4];
    nearest_record(sc, qt, holder, p, rec);
    if constexpr(kGrid) {
        out_distance[item] = rec[0].x;
        if(out_object != nullptr) {
            out_object[item] = (int32_t)__float_as_uint(rec[0].y);
        }
    }
    else {
        float4 *o = out + 4 * item;
        o[0] = rec[0];
        o[1] = rec[1];
        o[2] = rec[2];
        o[3] = rec[3];
    }
    if(counts != nullptr) {
        atomicAdd(counts, (unsigned long long)visits[0]);
        atomicAdd(counts + 1, (unsigned long long)visits[1]);
    }
}

} // namespace

#endif // PT_NEAREST_FUNCTIONS_ONLY

#endif
