// TEST ONLY: pt_face_table_kernel (pt_motion_shapes_kernels.h) behind the batched mesh assembler's own chain (pt_mesh_batch_kernels.h),
// both compiled for the HOST against tests/hip/host_pose as tests/hip/pose_probe.hip compiles the assembler alone, so that the face table
// can be checked over several chunks where there is no GPU (tests/test_face_table_cpu.py).  The loop is assemble_batch's (pt_meshes.cpp).
#include "pt_mesh_batch_kernels.h"
#include "pt_motion_shapes_kernels.h"

#include <algorithm>
#include <numeric>
#include <vector>

hipError_t pt_mesh_batch_scan(void *temp, size_t *bytes, const uint32_t *in, uint32_t *out, uint32_t n, hipStream_t) {
    if(temp == nullptr) {
        *bytes = 1;
        return hipSuccess;
    }
    std::exclusive_scan(in, in + n, out, 0u);
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

// The instances through pt_mesh_batch_chunk, chunked by the given limits (0 = the product's), with pt_face_table_launch behind every
// chunk.  pos / nrm / face_of have room for `room` triangles.  Returns 0, or 1000 + the HIP error; *chunks counts the chunks.
int face_table_probe(const ProbeMesh *meshes, const ProbeInstance *instances, uint32_t n_instances, uint64_t max_vertices, uint64_t max_faces, uint64_t max_corners, uint64_t room,
                     float *pos, float *nrm, uint32_t *face_of, uint32_t *counts, uint64_t *kept, uint32_t *chunks) {
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
    *kept = 0;
    *chunks = 0;
    uint64_t face_base_scene = 0;
    for(uint32_t first = 0; first < n_instances;) {
        const uint32_t end = pt_mesh_batch_chunk_end(nv.data(), nf.data(), n_instances, first, limits);
        uint64_t k = 0;
        hipError_t e = pt_mesh_batch_chunk(nullptr, scratch, table.data() + first, end - first, room - *kept, pos + 9 * *kept, nrm != nullptr ? nrm + 9 * *kept : nullptr,
                                           counts + first, &k, nullptr);
        if(e != hipSuccess) {
            return 1000 + static_cast<int>(e);
        }
        uint64_t chunk_faces = 0;
        for(uint32_t i = first; i < end; i++) {
            chunk_faces += nf[i];
        }
        if(chunk_faces > 0) {
            e = pt_face_table_launch(nullptr, static_cast<const uint32_t *>(scratch.flag.ptr), static_cast<const uint32_t *>(scratch.rank.ptr), static_cast<uint32_t>(chunk_faces),
                                     room - *kept, face_of + *kept, static_cast<uint32_t>(face_base_scene));
            if(e != hipSuccess) {
                return 1000 + static_cast<int>(e);
            }
        }
        face_base_scene += chunk_faces;
        *kept += k;
        ++*chunks;
        first = end;
    }
    return 0;
}

} // extern "C"
