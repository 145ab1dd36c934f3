// TEST ONLY: the batched mesh assembler's own source (pt_mesh_batch_kernels.h: kernels and launch chain) compiled for the HOST against
// tests/hip/host_pose, so that it runs where there is no GPU (tests/test_pose_batch_cpu.py).  The two library steps the device takes from
// hipcub are the standard library's here: an exclusive scan and a stable sort by key over the low end_bit bits.
#include "pt_mesh_batch_kernels.h"

#include <algorithm>
#include <numeric>
#include <vector>

static int g_scans = 0, g_sorts = 0;

hipError_t pt_mesh_batch_scan(void *temp, size_t *bytes, const uint32_t *in, uint32_t *out, uint32_t n, hipStream_t) {
    if(temp == nullptr) {
        *bytes = 1;
        return hipSuccess;
    }
    std::exclusive_scan(in, in + n, out, 0u);
    g_scans++;
    return hipSuccess;
}

hipError_t pt_mesh_batch_sort(void *temp, size_t *bytes, const uint32_t *keys_in, uint32_t *keys_out, const uint32_t *values_in, uint32_t *values_out, uint32_t n, int end_bit,
                              hipStream_t) {
    if(temp == nullptr) {
        *bytes = 1;
        return hipSuccess;
    }
    const uint32_t mask = end_bit >= 32 ? 0xffffffffu : (1u << end_bit) - 1u;
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return (keys_in[a] & mask) < (keys_in[b] & mask); });
    for(uint32_t i = 0; i < n; i++) {
        keys_out[i] = keys_in[order[i]];
        values_out[i] = values_in[order[i]];
    }
    g_sorts++;
    return hipSuccess;
}

struct ProbeMesh {
    uint32_t n_vertices;
    const float *vertices;
    uint32_t n_faces;
    const int32_t *faces;
};

struct ProbeInstance {
    uint32_t mesh;
    float transform[16];
    int32_t smooth;
};

extern "C" {

// The instances through pt_mesh_batch_chunk, chunked by the given limits (0 = the product's).  pos / nrm have room for `room` triangles.
// Returns 0, or 1000 + the HIP error; *chunks, *scans and *sorts count what ran.
int pose_probe_assemble(const ProbeMesh *meshes, const ProbeInstance *instances, uint32_t n_instances, uint64_t max_vertices, uint64_t max_faces, uint64_t max_corners,
                        uint64_t room, float *pos, float *nrm, uint32_t *counts, uint64_t *kept, uint32_t *chunks, uint32_t *scans, uint32_t *sorts) {
    std::vector<PtBatchInstance> table(n_instances);
    std::vector<uint32_t> nv(n_instances), nf(n_instances);
    for(uint32_t i = 0; i < n_instances; i++) {
        const ProbeMesh &m = meshes[instances[i].mesh];
        PtBatchInstance &t = table[i];
        t.vertices = m.vertices;
        t.faces = m.faces;
        t.n_vertices = nv[i] = m.n_vertices;
        t.n_faces = nf[i] = m.n_faces;
        t.vertex_base = t.face_base = 0;
        t.smooth = instances[i].smooth != 0 ? 1u : 0u;
        t.pad = 0;
        std::copy(instances[i].transform, instances[i].transform + 16, t.m);
    }
    PtBatchLimits limits;
    if(max_vertices != 0) {
        limits.max_vertices = max_vertices;
    }
    if(max_faces != 0) {
        limits.max_faces = max_faces;
    }
    if(max_corners != 0) {
        limits.max_corners = max_corners;
    }
    PtBatchScratch scratch;
    g_scans = g_sorts = 0;
    *kept = 0;
    *chunks = 0;
    for(uint32_t first = 0; first < n_instances;) {
        const uint32_t end = pt_mesh_batch_chunk_end(nv.data(), nf.data(), n_instances, first, limits);
        uint64_t k = 0;
        const hipError_t e = pt_mesh_batch_chunk(nullptr, scratch, table.data() + first, end - first, room - *kept, pos + 9 * *kept, nrm != nullptr ? nrm + 9 * *kept : nullptr,
                                                 counts + first, &k, nullptr);
        if(e != hipSuccess) {
            return 1000 + static_cast<int>(e);
        }
        *kept += k;
        ++*chunks;
        first = end;
    }
    *scans = static_cast<uint32_t>(g_scans);
    *sorts = static_cast<uint32_t>(g_sorts);
    return 0;
}

// kb_fill_ranges over the triangles [first_tri, first_tri + n) of arrays that hold first_tri + n entries
int pose_probe_fill_ranges(const PtBatchRange *ranges, uint32_t n_ranges, uint32_t first_tri, uint32_t n, uint32_t first_obj, uint8_t *tri_cull, uint32_t *tri_material,
                           uint32_t *tri_obj) {
    PtBatchScratch scratch;
    return static_cast<int>(pt_mesh_batch_fill_ranges(nullptr, scratch, ranges, n_ranges, first_tri, n, first_obj, tri_cull, tri_material, tri_obj));
}

} // extern "C"
