// TEST ONLY: query_record (pt_query_kernels.h; include/pt_query.h) compiled for the HOST against tests/hip/host_query,
// the way tests/hip/face_table_probe.hip compiles the face table's kernel, so that the record a walk's result becomes can be checked
// where there is no GPU (tests/test_query_cpu.py): it is fed the oracle's hits on scene tables the test lays out as pt_types.h says.
#define PT_QUERY_RECORD_ONLY
#include "pt_query_kernels.h"

#include <cstring>

extern "C" {

// tri_shade: [n_tris][8] float4, spheres [n_spheres] float4, sph_meta [n_spheres] (material, object); instances: [n_inst]
// PtQueryInstance; face_of: null or one word per instance triangle.  Query i: the hit (ref[i], t[i]) of the ray rays6[i].
// out: [n][16] words, the four vectors of every record.
int query_probe_records(uint32_t n_tris, const float *tri_shade, uint32_t n_spheres, const float *spheres, const uint32_t *sph_meta, const void *instances, uint32_t n_inst,
                        uint32_t first_object, const uint32_t *face_of, uint64_t n, const uint32_t *ref, const float *t, const float *rays6, float *out) {
    PtDevScene sc;
    memset(&sc, 0, sizeof(sc));
    sc.tri_shade = reinterpret_cast<const float4 *>(tri_shade);
    sc.spheres = reinterpret_cast<const float4 *>(spheres);
    sc.sph_meta = reinterpret_cast<const uint2 *>(sph_meta);
    sc.n_tris = n_tris;
    sc.n_spheres = n_spheres;
    PtQueryTables qt;
    qt.inst = static_cast<const PtQueryInstance *>(instances);
    qt.n_inst = n_inst;
    qt.first_object = first_object;
    qt.face_of = face_of;
    for(uint64_t i = 0; i < n; i++) {
        const float *r = rays6 + 6 * i;
        float4 rec[4];
        ptd::query_record(sc, qt, ref[i], t[i], ptd::v3(r[0], r[1], r[2]), ptd::v3(r[3], r[4], r[5]), rec);
        memcpy(out + 16 * i, rec, 64);
    }
    return 0;
}

int query_probe_sizes(uint32_t *instance_bytes) {
    *instance_bytes = sizeof(PtQueryInstance);
    return 0;
}

} // extern "C"
