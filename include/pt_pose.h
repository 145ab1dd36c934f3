/* pt_pose.h -- re-posing the mesh instances of a scene in place.  Part of the C ABI of libpathtrace_hip.so:
 * include/pt_hip.h includes this file behind pt_mesh.h, which it needs; it is not meant to be included on its own.
 *
 * A scene of pt_scene_create_meshes with at least one instance keeps what a new pose needs: its used meshes in device memory (12 bytes per
 * vertex + 12 bytes per face, once per mesh however many instances use it), its instance table (80 bytes per instance) and a host copy of
 * the description (what the caller's arrays held: 36 or 72 bytes per triangle of the description, 16 per sphere, 64 per material).  Behind
 * the first pose it also keeps the assembler's scratch in device memory -- 12 bytes per vertex and 8 per face of all instances, and 20
 * bytes per face corner (60 per face) if any instance is smooth -- and one spare position array and normal array (36 bytes per triangle
 * each), so that a pose of a scene that has been posed before allocates no scratch.  For the relight entry of pt_relight.h it keeps the
 * depth-first order of its leaves in device memory as well, 4 bytes per object.  Scenes without instances keep nothing of this.
 *
 *   - pt_scene_pose: replaces the matrices of the instances named by `instances` (n indices; NULL = all of them in order, and then n must
 *     be the scene's instance count) with transforms[k][16].  An index that occurs more than once gets the last of its matrices.  All
 *     instances are then assembled again by ONE chain of launches over their concatenated vertices and faces, and the tree is rebuilt (it
 *     keeps the reference's topology: there is no refit).  After the call the scene is, through every entry point (pt_scene_info,
 *     pt_scene_bvh_dump, pt_scene_emissive, pt_scene_instance_ranges, pt_scene_get_triangles, pt_intersect_batch, every render and
 *     feature entry), bit for bit the scene a fresh pt_scene_create_meshes gives for the same description, meshes, smooth and cull flags
 *     and materials with the new matrices, on the same device, under the environment at the time of the call (PT_BUILD and
 *     PT_BUILD_DEVICE_MIN are read anew).  Survivor counts, object ranges, the number of emitters, the depth of the tree and the builder
 *     may all change.  The scene keeps its address, its stream and its render workspace.
 *     The new content is built aside and adopted only when it is complete: a pose that fails leaves the scene as it was.
 *     PT_ERR_INVALID: a null scene; null transforms with n > 0; an index >= the instance count; instances == NULL with another n than
 *     the instance count; a scene with a live pt_frame (a frame's parked state belongs to the geometry it was created on: destroy the
 *     frames first).  PT_ERR_UNSUPPORTED: a scene without instances.  All of these before any device work.
 *     The call holds the scene's render lock: it waits for a render call in flight and none starts while it runs.
 *     `info` (may be NULL) receives what the pose did.
 *   - pt_scene_get_pose: the current matrices of all instances, [n_instances][16].  PT_ERR_UNSUPPORTED for a scene without instances.
 *   - pt_mesh_assemble_batch: the batched assembler on its own, without a scene or a tree: steps 1 - 3 of pt_mesh.h for every instance
 *     (material and cull_backface are not read), the survivors of instance 0, 1, ... end to end: their number to *n_triangles, the
 *     per-instance numbers to out_counts[n_instances] (may be NULL) and the first min(*n_triangles, capacity) triangles to out_pos /
 *     out_nrm ([capacity][9] each; face normals for the instances that are not smooth).  Nothing is written past `capacity` triangles.
 *     PT_ERR_INVALID: a null pointer (out_pos / out_nrm may be NULL when capacity is 0), an instance whose mesh is >= n_meshes, a used mesh
 *     with a missing array.  PT_ERR_UNSUPPORTED: a used mesh with more than 715,827,882 faces, or more than 2^30 - 1 faces over all
 *     instances.  All before any device work; then PT_ERR_NO_DEVICE. */
#ifndef PT_POSE_ABI_H
#define PT_POSE_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_pose_info {
    uint32_t n_instances, n_triangles; /* instances of the scene; surviving instance triangles after this pose */
    uint32_t assembly_syncs;           /* host waits on the device inside the assembly: one per chunk */
    uint32_t assembly_chunks;          /* 1 unless one batch would exceed 2^31 - 1 corners or 2^32 - 1 vertices or faces */
    float upload_ms, assembly_ms, tree_ms, rest_ms, total_ms; /* device events for assembly and tree, wall clock otherwise */
} pt_pose_info;

int pt_scene_pose(pt_scene *scene, const uint32_t *instances, uint32_t n, const float *transforms /* [n][16], rows */, pt_pose_info *info /* may be NULL */);
int pt_scene_get_pose(const pt_scene *scene, float *transforms /* [n_instances][16] */);
int pt_mesh_assemble_batch(int device, const pt_mesh_data *meshes, uint32_t n_meshes, const pt_mesh_instance *instances, uint32_t n_instances, uint64_t capacity,
                           float *out_pos, float *out_nrm, uint32_t *out_counts /* [n_instances] */, uint64_t *n_triangles);

#ifdef __cplusplus
}
#endif

#endif
