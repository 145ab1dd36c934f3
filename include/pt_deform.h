/* pt_deform.h -- deforming the meshes of a scene in place: new vertices from the caller, or linear blend skinning on the device
 * (DESIGN.md 4.3.4).  Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h includes this file behind pt_pose.h, whose scenes it
 * works on; it is not meant to be included on its own.
 *
 * A scene of pt_scene_create_meshes with at least one instance keeps its used meshes in device memory (pt_pose.h): their REST vertices.
 * A deformation gives a mesh CURRENT vertices beside them, in a device buffer of its own, and the assembler reads those instead.  ALL
 * INSTANCES OF A MESH SHARE ITS DEFORMATION: two characters that bend differently are two meshes of the creating call, even when their
 * rest vertices and faces are equal.  The faces never change.
 *
 * Memory, on top of pt_pose.h: a bound skin is 8 * K bytes per vertex (K bone indices and K weights); a mesh that has been deformed keeps
 * its current vertices and the spare buffer the next deformation is made in (a failed call must leave the current ones as they were),
 * 12 bytes per vertex each, allocated by the mesh's first deformation and reused by every later one; a call with skinned meshes keeps one
 * bone table of 48 bytes per bone of the largest rig.  PT_DEFORM_REST frees nothing.  A scene that is never deformed keeps none of this
 * and takes exactly the path it took before this header existed.
 *
 *   - pt_scene_bind_skin: binds a rig to one mesh: for every vertex K = `influences` bone indices and K weights.  The weights are used as
 *     given: not normalised, any sign, zero allowed.  Everything is checked on the host before any device work, EVERY BONE INDEX
 *     INCLUDED: no index >= n_bones ever reaches the device, and the kernel checks none.  The arrays are then uploaded once; a mesh has
 *     one skin, a new one replaces it.  n_bones == 0 or bone == NULL unbinds.  Binding changes no geometry, not even that of a mesh that
 *     is skinned at the moment: the next PT_DEFORM_BONES uses the new rig.
 *     PT_ERR_INVALID: a null scene or skin; `influences` outside 1 .. PT_SKIN_MAX_INFLUENCES; a null weight array; a mesh index out of
 *     range or a mesh no instance uses; a bone index >= n_bones; a scene with a live pt_frame, as for a pose.  PT_ERR_UNSUPPORTED: a scene
 *     without instances.  The call holds the scene's render lock.
 *   - pt_scene_deform does three things in order.
 *     1. Every mesh named in deforms[n_deforms] gets current vertices according to `kind`:
 *          PT_DEFORM_VERTICES  data[n_vertices][3] is uploaded;
 *          PT_DEFORM_BONES     data[n_bones][12] are rows 0 .. 2 of every bone's mat4, and vertex i becomes
 *                                  sum over k = 0 .. K-1, in order, of weight[i][k] * (B(bone[i][k]) * (x, y, z, 1))
 *                              of its REST vertex (x, y, z): skinning never compounds.  Per component c: acc = 0; per influence
 *                              d = 0, d += B[c][0]*x, d += B[c][1]*y, d += B[c][2]*z, d += B[c][3]*1 (the dot of the assembler's
 *                              transform), acc += weight * d, every product and sum rounded to float on its own.  No influence is
 *                              skipped, a zero weight included (0 * inf and 0 * NaN are NaN, as IEEE 754 says); there is no division
 *                              by a w.  One kernel launch per skinned mesh on the scene's stream, no host wait before the assembly;
 *          PT_DEFORM_REST      the mesh goes back to the vertices it was created with (data is not read, count is not checked).
 *        A mesh named more than once takes its last entry.
 *     2. The instances named by `instances` get transforms[n][16] exactly as by pt_scene_pose; n == 0: the pose stays.
 *     3. What a pose does: ONE batched assembly over all instances -- reading the current vertices of the deformed meshes and the rest
 *        vertices of the others -- and the tree rebuilt aside, adopted only when it is complete.
 *     After the call the scene is, through every entry point (those pt_pose.h lists), bit for bit the scene a fresh
 *     pt_scene_create_meshes gives for the same description, faces, flags and materials, the current matrices, and meshes whose vertices
 *     are what pt_scene_get_mesh_vertices returns, on the same device under the environment at the time of the call.  Vertices that are
 *     NaN or infinite reject their faces in the assembler's face test like any others; survivor counts, object ranges and emitters follow.
 *     A later pt_scene_pose or pt_scene_relight works on the deformed shape.
 *     A call that fails leaves the scene AND the current vertices of every mesh as they were: new vertices are made in the spare buffers
 *     and swapped in on success.
 *     PT_ERR_INVALID: a null scene; null deforms with n_deforms > 0; an unknown kind; null data for VERTICES or BONES; a mesh index out of
 *     range or a mesh no instance uses; a count other than the mesh's vertex count (VERTICES) or its skin's bone count (BONES); BONES for
 *     a mesh without a bound skin; and, word for word as for pt_scene_pose: null transforms with n > 0; an index >= the instance count;
 *     instances == NULL with another n than 0 or the instance count; a scene with a live pt_frame (a frame's parked state belongs to the
 *     geometry it was created on: destroy the frames first).  PT_ERR_UNSUPPORTED: a scene without instances.  All of these before any
 *     device work.  The call holds the scene's render lock: it waits for a render call in flight and none starts while it runs.
 *     `info` (may be NULL) receives what the call did.
 *   - pt_scene_get_mesh_vertices: the vertices the assembler reads for `mesh` at the moment, [n_vertices][3]: the current ones of a
 *     deformed mesh, the rest ones otherwise.  *n_vertices (may be NULL) receives their number; out == NULL asks for the number alone.
 *     PT_ERR_INVALID: a null scene, a mesh out of range or unused.  PT_ERR_UNSUPPORTED: a scene without instances.
 *
 * OUT OF SCOPE: motion vectors of a deformed mesh are not made here.  pt_render_features_motion (pt_motion.h) describes a deformed mesh
 * by its instance matrix alone; pt_scene_motion_mark and pt_render_features_motion_marked (pt_motion_shapes.h) remember the shape every
 * mesh had at the previous frame and reproject a hit through the vertices of its face.  Every successful pt_scene_deform bumps the shape
 * serial of the meshes it names, which is how a mark knows that a mesh changed. */
#ifndef PT_DEFORM_ABI_H
#define PT_DEFORM_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

#define PT_SKIN_MAX_INFLUENCES 8

#define PT_DEFORM_VERTICES 0u
#define PT_DEFORM_BONES 1u
#define PT_DEFORM_REST 2u

typedef struct pt_skin {   /* a rig bound to one mesh of the scene */
    uint32_t mesh;         /* mesh index of the creating pt_scene_create_meshes call */
    uint32_t n_bones;      /* >= 1 (0: unbind) */
    uint32_t influences;   /* K, 1 .. PT_SKIN_MAX_INFLUENCES, the same for every vertex */
    const uint32_t *bone;  /* [n_vertices][K], each < n_bones (NULL: unbind) */
    const float *weight;   /* [n_vertices][K], used as given: not normalised, any sign, 0 allowed */
} pt_skin;

typedef struct pt_mesh_deform { /* one mesh's new shape */
    uint32_t mesh;
    uint32_t kind;         /* PT_DEFORM_VERTICES | PT_DEFORM_BONES | PT_DEFORM_REST */
    const float *data;     /* VERTICES: [n_vertices][3];  BONES: [n_bones][12], rows 0..2 of each bone's mat4;  REST: NULL */
    uint32_t count;        /* n_vertices or n_bones: must match, else PT_ERR_INVALID */
} pt_mesh_deform;

typedef struct pt_deform_info {
    uint32_t n_instances, n_triangles; /* the fields of pt_pose_info, with its meanings ... */
    uint32_t assembly_syncs;
    uint32_t assembly_chunks;
    float upload_ms, assembly_ms, tree_ms, rest_ms, total_ms; /* (upload_ms: the description's triangles, as for a pose) */
    uint32_t n_meshes_deformed;        /* ... meshes that got new current vertices or went back to rest (a mesh named twice counts once) */
    uint32_t n_vertices_skinned;       /* vertices the skinning kernel made */
    float skin_ms;                     /* device events around the skinning launches */
    float vertex_upload_ms;            /* wall clock of the uploads of PT_DEFORM_VERTICES arrays and bone tables */
    uint32_t allocations;              /* device allocations of the assembler's scratch and of vertex and bone buffers so far, this call's included */
} pt_deform_info;

int pt_scene_bind_skin(pt_scene *scene, const pt_skin *skin);
int pt_scene_deform(pt_scene *scene, const pt_mesh_deform *deforms, uint32_t n_deforms, const uint32_t *instances, uint32_t n,
                    const float *transforms /* [n][16], rows */, pt_deform_info *info /* may be NULL */);
int pt_scene_get_mesh_vertices(pt_scene *scene, uint32_t mesh, float *out /* [n_vertices][3] */, uint32_t *n_vertices);

#ifdef __cplusplus
}
#endif

#endif
