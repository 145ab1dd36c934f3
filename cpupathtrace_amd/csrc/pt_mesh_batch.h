// pt_mesh_batch.h -- the mesh assembler: indexed meshes under transforms, expanded into triangle arrays in device memory, all instances
// of a call through ONE chain of launches (pt_mesh_batch.hip, kernels in pt_mesh_batch_kernels.h, where the steps are described;
// DESIGN.md 4.3.1 and 4.3.2).  The chain works over the concatenated vertices and faces of a chunk of instances, driven by an instance
// table in device memory.  An instance's triangles do not depend on what else is in its chunk: they are, bit for bit, what io::loadMesh
// makes of that mesh under that matrix.
#ifndef PT_MESH_BATCH_H
#define PT_MESH_BATCH_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>

// One entry of the instance table.  vertex_base / face_base: the instance's first vertex / face in the chunk's concatenated index spaces
struct PtBatchInstance {
    const float *vertices;  // device, [n_vertices][3], untransformed
    const int32_t *faces;   // device, [n_faces][3]
    uint32_t n_vertices, n_faces;
    uint32_t vertex_base, face_base;
    uint32_t smooth, pad;
    float m[16];            // rows of the mat4
};

// cull / material of the triangles [first_tri, first_tri + count); sorted by first_tri, empty ranges allowed
struct PtBatchRange {
    uint32_t first_tri, count, material, cull;
};

// The most vertices, faces and corners of one chunk: the corner list (3 per face) is sorted with 32-bit counts and the key of a flat
// instance's corners is the chunk's vertex count itself
struct PtBatchLimits {
    uint64_t max_vertices = 0xffffffffull, max_faces = 0xffffffffull, max_corners = 0x7fffffffull;
};

// Device scratch of the chain, grown on demand and never shrunk: a pose of a scene that has been posed before allocates nothing.  It
// may be released only when the streams that were given it have been waited for
struct PtBatchScratch {
    struct Buf {
        void *ptr = nullptr;
        size_t bytes = 0;
    };
    Buf table, tv, flag, rank, counts, unit, corner_vertex, corner_id, sorted_vertex, sorted_id, temp, ranges;
    uint64_t allocations = 0; // hipMalloc calls so far
    PtBatchScratch() = default;
    PtBatchScratch(const PtBatchScratch &) = delete;
    PtBatchScratch &operator=(const PtBatchScratch &) = delete;
    ~PtBatchScratch() { release(); }
    hipError_t ensure(Buf &b, size_t bytes) {
        if(b.ptr != nullptr && bytes <= b.bytes) {
            return hipSuccess;
        }
        if(b.ptr != nullptr) {
            (void)hipFree(b.ptr);
            b.ptr = nullptr;
            b.bytes = 0;
        }
        const size_t want = bytes > 0 ? bytes : 1;
        const hipError_t e = hipMalloc(&b.ptr, want);
        if(e == hipSuccess) {
            b.bytes = want;
            allocations++;
        }
        else {
            b.ptr = nullptr;
        }
        return e;
    }
    void release() {
        for(Buf *b : {&table, &tv, &flag, &rank, &counts, &unit, &corner_vertex, &corner_id, &sorted_vertex, &sorted_id, &temp, &ranges}) {
            if(b->ptr != nullptr) {
                (void)hipFree(b->ptr);
                b->ptr = nullptr;
                b->bytes = 0;
            }
        }
    }
};

// The end (exclusive) of the chunk that starts at instance `first`: as many consecutive instances as the limits allow, one at least.
// n_vertices / n_faces: per instance.  Host only.
uint32_t pt_mesh_batch_chunk_end(const uint32_t *n_vertices, const uint32_t *n_faces, uint32_t n_instances, uint32_t first, const PtBatchLimits &limits);

// One chunk: `table` (host memory; vertex_base and face_base are filled in here) names n_instances instances.  Their survivors are written
// end to end, in instance and face order, to pos[k][9] and nrm[k][9] (k < room; nrm may be null when no instance is smooth), the
// per-instance counts to counts[n_instances] (host) and their sum to *kept.  Waits for the stream ONCE, to read the counts; what follows
// the wait (corner sort, smoothing) is only enqueued: the caller orders its readers behind the stream.  `table` and `counts` must stay
// valid until then.  Returns hipSuccess or the first error; `what` (optional) receives a static description of the failing step.
hipError_t pt_mesh_batch_chunk(hipStream_t stream, PtBatchScratch &scratch, PtBatchInstance *table, uint32_t n_instances, uint64_t room, float *pos, float *nrm,
                               uint32_t *counts, uint64_t *kept, const char **what);

// cull / material / object index of the triangles [first_tri, first_tri + n) from the range table (host memory, uploaded here with a
// blocking copy), in one launch: triangle t is object first_obj + (t - first_tri)
hipError_t pt_mesh_batch_fill_ranges(hipStream_t stream, PtBatchScratch &scratch, const PtBatchRange *ranges, uint32_t n_ranges, uint32_t first_tri, uint32_t n,
                                     uint32_t first_obj, uint8_t *tri_cull, uint32_t *tri_material, uint32_t *tri_obj);

// The two library steps of the chain (pt_mesh_batch.hip: hipcub; the host build of tests/hip/pose_probe.hip: the standard library).
// temp == nullptr: *bytes receives the temporary storage n items need.
hipError_t pt_mesh_batch_scan(void *temp, size_t *bytes, const uint32_t *in, uint32_t *out, uint32_t n, hipStream_t stream);
hipError_t pt_mesh_batch_sort(void *temp, size_t *bytes, const uint32_t *keys_in, uint32_t *keys_out, const uint32_t *values_in, uint32_t *values_out, uint32_t n, int end_bit,
                              hipStream_t stream);

#endif
