// pt_motion_shapes_kernels.h -- which face every instance triangle came from (include/pt_motion_shapes.h).  Included by
// exactly one translation unit (pt_walks.hip; tests/hip/face_table_probe.hip compiles it for the host).
//
// The assembler (pt_mesh_batch_kernels.h) keeps a chunk's faces that pass its test in face order, so the exclusive rank of a kept face
// IS its triangle index inside the chunk.  pt_mesh_batch_chunk leaves the chunk's flags and ranks in its scratch (the corner sort and the
// smoothing that may still be in flight use other buffers), and pt_face_table_kernel, launched on the same stream right behind it, turns
// them into the table: one thread per chunk face f,
//     flag[f] != 0 and rank[f] < room:  face_of[rank[f]] = face_base_scene + f
// where face_of points at the chunk's first triangle and face_base_scene is the number of faces in the chunks before.  Nothing else is
// written: a rejected face has no triangle.  The assembler's kernels and pt_mesh_batch_chunk are not touched.
#ifndef PT_MOTION_SHAPES_KERNELS_H
#define PT_MOTION_SHAPES_KERNELS_H

#include <hip/hip_runtime.h>

#include <cstdint>

__global__ void pt_face_table_kernel(uint32_t n_faces, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, uint64_t room, uint32_t *__restrict__ face_of,
                                     uint32_t face_base_scene) {
    const uint64_t f = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if(f >= n_faces || flag[f] == 0u) {
        return;
    }
    const uint64_t j = rank[f];
    if(j >= room) { // (as kb_expand: nothing is written for a triangle there is no room for)
        return;
    }
    face_of[j] = face_base_scene + static_cast<uint32_t>(f);
}

hipError_t pt_face_table_launch(hipStream_t stream, const uint32_t *flag, const uint32_t *rank, uint32_t n_faces, uint64_t room, uint32_t *face_of, uint32_t face_base_scene) {
    if(n_faces == 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(pt_face_table_kernel, dim3(static_cast<unsigned>((static_cast<uint64_t>(n_faces) + 255) / 256)), dim3(256), 0, stream, n_faces, flag, rank, room, face_of,
                       face_base_scene);
    return hipGetLastError();
}

#endif
