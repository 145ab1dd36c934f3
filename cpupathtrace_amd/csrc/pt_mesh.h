// pt_mesh.h -- indexed meshes instantiated under transforms, expanded into triangle arrays ON the device (pt_mesh.hip): what
// io::loadMesh does after it has read the numbers.  The arrays it fills are the ones pt_build.hip starts from (PtBuildInput).
#ifndef PT_MESH_H
#define PT_MESH_H

#include <hip/hip_runtime.h>

#include <cstdint>

// An indexed mesh in device memory
struct PtMeshDevice {
    uint32_t n_vertices = 0;
    const float *vertices = nullptr; // [n_vertices][3], untransformed
    uint32_t n_faces = 0;
    const int32_t *faces = nullptr;  // [n_faces][3], 0-based; any value (checked on the device)
};

// The most faces of one mesh pt_mesh_assemble_device takes: the corner list of the smoothing step (3 per face) is sorted with 32-bit counts
constexpr uint32_t PT_MESH_MAX_FACES = 0x7fffffffu / 3u;

// Transforms the vertices by `m16` (rows of a mat4, host memory), drops the faces io::loadMesh drops and writes the survivors in face
// order: positions to pos[k][9], normals to nrm[k][9] (k = 0 .. *n_kept - 1).  smooth: the normalised sums of the unit face normals
// around every vertex, added in ascending face order; otherwise face normals.  nrm may be null when !smooth.  pos and nrm must have room
// for mesh.n_faces triangles.  Synchronises the stream (the count is read back).  `device_ms`, if not null, receives the device time.
// Returns hipSuccess or the first HIP error; `what` (optional) receives a static description of the failing step.
hipError_t pt_mesh_assemble_device(hipStream_t stream, const PtMeshDevice &mesh, const float *m16, bool smooth, float *pos, float *nrm, uint32_t *n_kept, float *device_ms,
                                   const char **what);

// cull / material / object index of the triangles [first_tri, first_tri + count): one instance's constants, objects numbered from first_obj
hipError_t pt_mesh_fill_range(hipStream_t stream, uint32_t first_tri, uint32_t count, uint8_t cull, uint32_t material, uint32_t first_obj, uint8_t *tri_cull,
                              uint32_t *tri_material, uint32_t *tri_obj);

// Triangle::Triangle's normals for n triangles (the formula of k_triangle_records, pt_build.hip): nrm[t] = 3 x normalize(cross(b - a, c - a))
hipError_t pt_mesh_face_normals(hipStream_t stream, uint32_t n, const float *pos, float *nrm);

// out[i][9] = pos[idx[i]][9]
hipError_t pt_mesh_gather_pos(hipStream_t stream, const float *pos, const uint32_t *idx, uint32_t n, float *out);

// Triangles back out of a built scene: positions from the kept position array, normals, cull flag and material from the shading records
// (8 float4 per triangle, pt_types.h).  Triangle i of the output is idx[i], or first + i where idx is null.  Any output may be null.
hipError_t pt_mesh_unpack(hipStream_t stream, const float *pos, const float4 *shade, const uint32_t *idx, uint32_t first, uint32_t n, float *out_pos, float *out_nrm,
                          uint8_t *out_cull, uint32_t *out_material);

#endif
