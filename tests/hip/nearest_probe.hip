// TEST ONLY: the device functions of the nearest-surface queries (pt_nearest_kernels.h; include/pt_nearest.h) compiled
// for the HOST against tests/hip/host_query, the way tests/hip/query_probe.hip compiles query_record, so that the per-triangle and
// per-sphere arithmetic, the pruning bound and the record can be checked where there is no GPU (tests/test_nearest_cpu.py).
#define PT_NEAREST_FUNCTIONS_ONLY
#include "pt_nearest_kernels.h"

#include "../../include/pt_hip.h"

#include <cstddef>
#include <cstring>

extern "C" {

// n pairs (p[i], triangle (a, ab, ac)[i]): out[i] = (d2, v, w, bits feature, diff xyz, 0)
int nearest_probe_triangles(uint64_t n, const float *p, const float *a, const float *ab, const float *ac, float *out) {
    for(uint64_t i = 0; i < n; i++) {
        ptd::V3 diff;
        const ptd::NearestHit h = ptd::nearest_triangle(ptd::ld3(a + 3 * i), ptd::ld3(ab + 3 * i), ptd::ld3(ac + 3 * i), ptd::ld3(p + 3 * i), diff);
        float *o = out + 8 * i;
        o[0] = h.d2;
        o[1] = h.v;
        o[2] = h.w;
        o[3] = __uint_as_float(h.feature);
        o[4] = diff.x;
        o[5] = diff.y;
        o[6] = diff.z;
        o[7] = 0.0f;
    }
    return 0;
}

// n pairs (p[i], sphere (c, R)[i]): out[i] = (d2, len, dist, bits feature)
int nearest_probe_spheres(uint64_t n, const float *p, const float *sph4, float *out) {
    for(uint64_t i = 0; i < n; i++) {
        ptd::V3 pc;
        float len, dist;
        const ptd::NearestHit h = ptd::nearest_sphere(ptd::ld3(sph4 + 4 * i), sph4[4 * i + 3], ptd::ld3(p + 3 * i), pc, len, dist);
        float *o = out + 4 * i;
        o[0] = h.d2;
        o[1] = len;
        o[2] = dist;
        o[3] = __uint_as_float(h.feature);
    }
    return 0;
}

// n triples (p[i], box (lo, hi)[i]) with the margin m[i]: out[i] = the pruning rule's bound
int nearest_probe_bounds(uint64_t n, const float *p, const float *lo, const float *hi, const float *m, float *out) {
    for(uint64_t i = 0; i < n; i++) {
        out[i] = ptd::nearest_box_bound(ptd::ld3(lo + 3 * i), ptd::ld3(hi + 3 * i), ptd::ld3(p + 3 * i), m[i]);
    }
    return 0;
}

// m of n points for the root box (root_lo, root_hi)
int nearest_probe_margins(uint64_t n, const float *p, const float *root_lo, const float *root_hi, float *out) {
    for(uint64_t i = 0; i < n; i++) {
        out[i] = ptd::nearest_margin(root_lo, root_hi, ptd::ld3(p + 3 * i));
    }
    return 0;
}

// The answers of n queries (xyz, max_distance) by the kernel's own leaf code and take rule over EVERY leaf record in turn -- no tree,
// no pruning --, and their records.  recs: [n_tris + 1 + n_spheres][4] float4 as pt_types.h lays the leaf records out; sph_meta
// [n_spheres] (material, object); instances: [n_inst] PtQueryInstance; face_of: null or one word per instance triangle.  out: [n][16]
// words.  `order`: the leaf records in the order they are offered (a permutation of the n_tris + n_spheres record indices).
int nearest_probe_records(uint32_t n_tris, uint32_t n_spheres, const float *recs, const uint32_t *sph_meta, const void *instances, uint32_t n_inst, uint32_t first_object,
                          const uint32_t *face_of, const uint32_t *order, uint64_t n, const float *points4, float *out) {
    PtDevScene sc;
    memset(&sc, 0, sizeof(sc));
    sc.recs = reinterpret_cast<const float4 *>(recs);
    sc.sph_meta = reinterpret_cast<const uint2 *>(sph_meta);
    sc.n_tris = n_tris;
    sc.n_spheres = n_spheres;
    PtQueryTables qt;
    qt.inst = static_cast<const PtQueryInstance *>(instances);
    qt.n_inst = n_inst;
    qt.first_object = first_object;
    qt.face_of = face_of;
    for(uint64_t i = 0; i < n; i++) {
        const float *q = points4 + 4 * i;
        const ptd::V3 p = ptd::v3(q[0], q[1], q[2]);
        const float r = q[3];
        uint32_t holder = PT_REF_NONE;
        if(r >= 0.0f && p.x == p.x && p.y == p.y && p.z == p.z) {
            float best = r * r;
            for(uint32_t k = 0; k < n_tris + n_spheres; k++) {
                const uint32_t index = order[k];
                const float4 *rec = sc.recs + 4 * (size_t)index;
                float d2;
                uint32_t ref = PT_REF_LEAF | index;
                if(index > n_tris) {
                    ptd::V3 pc;
                    float len, dist;
                    d2 = ptd::nearest_sphere(ptd::v3(rec[0].x, rec[0].y, rec[0].z), rec[0].w, p, pc, len, dist).d2;
                    ref |= PT_REF_SPHERE;
                }
                else {
                    const ptd::TriRec tri = ptd::tri_unpack(rec[0], rec[1], rec[2]);
                    ptd::V3 diff;
                    d2 = ptd::nearest_triangle(tri.a, tri.ab, tri.ac, p, diff).d2;
                }
                if(ptd::nearest_takes(d2, index, best, holder)) {
                    best = d2;
                    holder = ref;
                }
            }
        }
        float4 rec4[4];
        ptd::nearest_record(sc, qt, holder, p, rec4);
        memcpy(out + 16 * i, rec4, 64);
    }
    return 0;
}

int nearest_probe_sizes(uint32_t *record_bytes, uint32_t *grid_bytes, uint32_t *offsets /* [12] */) {
    *record_bytes = sizeof(pt_nearest);
    *grid_bytes = sizeof(pt_distance_grid);
    const size_t fields[12] = {offsetof(pt_nearest, distance), offsetof(pt_nearest, object), offsetof(pt_nearest, instance), offsetof(pt_nearest, face),
                               offsetof(pt_nearest, position), offsetof(pt_nearest, material), offsetof(pt_nearest, geometric_normal), offsetof(pt_nearest, b1),
                               offsetof(pt_nearest, squared_distance), offsetof(pt_nearest, feature), offsetof(pt_nearest, side), offsetof(pt_nearest, b2)};
    for(int k = 0; k < 12; k++) {
        offsets[k] = (uint32_t)fields[k];
    }
    return 0;
}

} // extern "C"
