// pt_mesh.h -- the small per-triangle kernels around a scene's triangle arrays in HBM (pt_mesh.hip).  The arrays are the ones the batched
// assembler fills from meshes and instances (pt_mesh_batch.h) and pt_build.hip starts from (PtBuildInput).
#ifndef PT_MESH_H
#define PT_MESH_H

#include <hip/hip_runtime.h>

#include <cstdint>

// The most faces of one mesh: the corner list of the smoothing step (3 per face) is sorted with 32-bit counts
constexpr uint32_t PT_MESH_MAX_FACES = 0x7fffffffu / 3u;

// Triangle::Triangle's normals for n triangles (the formula of k_triangle_records, pt_build.hip): nrm[t] = 3 x normalize(cross(b - a, c - a))
hipError_t pt_mesh_face_normals(hipStream_t stream, uint32_t n, const float *pos, float *nrm);

// out[i][9] = pos[idx[i]][9]
hipError_t pt_mesh_gather_pos(hipStream_t stream, const float *pos, const uint32_t *idx, uint32_t n, float *out);

// Triangles back out of a built scene: positions from the kept position array, normals, cull flag and material from the shading records
// (8 float4 per triangle, pt_types.h).  Triangle i of the output is idx[i], or first + i where idx is null.  Any output may be null.
hipError_t pt_mesh_unpack(hipStream_t stream, const float *pos, const float4 *shade, const uint32_t *idx, uint32_t first, uint32_t n, float *out_pos, float *out_nrm,
                          uint8_t *out_cull, uint32_t *out_material);

#endif
