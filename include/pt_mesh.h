/* pt_mesh.h -- scenes from indexed meshes and instances, assembled on the device.  Part of the C ABI of
 * libpathtrace_hip.so: include/pt_hip.h includes this file, which is not meant to be included on its own.
 *
 * A mesh is handed over once as vertices + faces and INSTANTIATED under transforms; the triangles are made in device memory.  The device
 * does everything io::loadMesh(stream, transformation, cull_backface, smooth) does after it has read the numbers
 * (reference src/scene/mesh.cpp, include/PathTrace/util/matrix.h):
 *   1. v' = transform * (x, y, z, 1), row by row with the library's dot (sums start from zero), then times 1 / w'.  Projective rows and
 *      w' = 0 are legal: the resulting inf / NaN positions are rejected by step 2.
 *   2. a face is dropped, in face order, if an index lies outside [0, n_vertices), if |b-a|^2 > 0 && |c-a|^2 > 0 && |c-b|^2 > 0 is false
 *      (NaN rejects), or if |cross(b-a, c-a)|^2 <= 0 -- all on the TRANSFORMED vertices.  Survivors keep their relative order.
 *   3. smooth = 0: every corner has the face normal normalize(cross(b-a, c-a)) (Triangle::Triangle).  smooth = 1: per vertex, the unit
 *      normals of the surviving faces that use it are added in ascending face order starting from zero; if the sum's squared length
 *      is <= 0 the vertex's corners keep their face normals, otherwise they get the normalised sum (a NaN sum is normalised and assigned).
 * The result is bit for bit what pt_scene_create builds from the triangles io::loadMesh returns for the same vertices, faces and matrix:
 * tree, emitters, hits and pixels.  This is not instancing in the two-level sense: the tree keeps the reference's topology, so every
 * instance is fully expanded -- in device memory.  What goes away is the expansion on the host, the upload and the per-triangle objects.
 *
 *   - pt_scene_create_meshes: pt_scene_create for the objects of `desc` FOLLOWED BY the surviving triangles of instance 0, instance 1, ...
 *     Object indices (pt_intersect_batch, pt_scene_emissive, pt_scene_bvh_dump) follow this order.  Every mesh is uploaded once per call,
 *     however many instances use it.  An instance has one material (an index into desc->materials or PT_NO_MATERIAL) and one cull flag;
 *     an emissive material makes each of its triangles an emitter.  With n_instances == 0 the call is pt_scene_create.  Where
 *     desc->tri_nrm is NULL and a smooth instance needs the normal array, the desc's own triangles get their face normals on the device.
 *     A scene the device builds (PT_BUILD_DEVICE_MIN objects and more, or PT_BUILD=device) makes no host round trip of per-triangle data:
 *     only the instances' survivor counts and the records of the emissive triangles are read back.  The host builder downloads the
 *     assembled arrays and goes on as pt_scene_create does.
 *     PT_ERR_INVALID: a null pointer, an instance whose mesh is >= n_meshes or whose material is neither PT_NO_MATERIAL nor < n_materials.
 *     smooth and cull_backface are read as flags (0 / not 0).  PT_ERR_UNSUPPORTED: desc->n_triangles + the faces of all instances (before any is
 *     rejected) exceed 2^30 - 1, or one mesh has more than 715,827,882 faces.  Both before any device work; then PT_ERR_NO_DEVICE.
 *     Such a scene keeps the triangles' positions in device memory (36 bytes per triangle) for pt_scene_get_triangles.
 *   - pt_mesh_assemble: steps 1 - 3 for one instance (instance->mesh, material and cull_backface are not read), copied back: the number of
 *     surviving triangles to *n_triangles, and the first min(that, capacity) of them to out_pos / out_nrm ([capacity][9] each; face
 *     normals when !smooth).  Nothing is written past `capacity` triangles.
 *   - pt_scene_instance_ranges: the first object and the number of objects (surviving triangles) of every instance, n_instances entries each.
 *   - pt_scene_get_triangles: the triangle objects first_object .. first_object + count - 1 of a scene made by pt_scene_create_meshes with
 *     at least one instance, as the builder took them: out_pos, out_nrm [count][9], out_cull, out_material [count]; any of them may be
 *     NULL.  PT_ERR_INVALID for a range that leaves the scene or holds a sphere, PT_ERR_UNSUPPORTED for a scene of plain pt_scene_create. */
#ifndef PT_MESH_ABI_H
#define PT_MESH_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_mesh_data {
    uint32_t n_vertices;
    const float *vertices; /* [n_vertices][3], untransformed */
    uint32_t n_faces;
    const int32_t *faces;  /* [n_faces][3], 0-based */
} pt_mesh_data;

typedef struct pt_mesh_instance {
    uint32_t mesh;         /* index into the call's meshes */
    float transform[16];   /* rows, as mat4 */
    int32_t smooth;
    int32_t cull_backface;
    uint32_t material;     /* index into desc->materials or PT_NO_MATERIAL */
} pt_mesh_instance;

int pt_scene_create_meshes(int device, const pt_scene_desc *desc, const pt_mesh_data *meshes, uint32_t n_meshes, const pt_mesh_instance *instances,
                           uint32_t n_instances, pt_scene **out);
int pt_mesh_assemble(int device, const pt_mesh_data *mesh, const pt_mesh_instance *instance, uint64_t capacity, float *out_pos, float *out_nrm,
                     uint64_t *n_triangles);
int pt_scene_instance_ranges(const pt_scene *scene, uint32_t *first_object, uint32_t *n_objects);
int pt_scene_get_triangles(pt_scene *scene, uint32_t first_object, uint32_t count, float *out_pos, float *out_nrm, uint8_t *out_cull, uint32_t *out_material);

#ifdef __cplusplus
}
#endif

#endif
