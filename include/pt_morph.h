/* pt_morph.h -- blend shapes (morph targets) for the meshes of a scene, evaluated on the device, alone or in front of the skeleton
 * (DESIGN.md 4.3.5).  Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h includes this file behind pt_deform.h, whose buffers,
 * rigs and scenes it works on; it is not meant to be included on its own.
 *
 * A mesh of a scene with instances (pt_pose.h) gets a bound MORPH SET of T targets.  Target t is a list of (vertex, delta[3]) pairs:
 * sparse, with strictly ascending vertex indices each < n_vertices, or dense, with vertex == NULL, where n_deltas must equal n_vertices
 * and entry i belongs to vertex i.  An empty target (n_deltas == 0) is legal.  A morph call gives the mesh T weights and makes its
 * CURRENT vertices (pt_deform.h) from its REST vertices.  For vertex i and component c:
 *
 *     m = rest[i][c]
 *     for every target t that lists vertex i, in ascending t:   m += weight[t] * delta_t(i)[c]
 *
 * Product and sum are each one IEEE float operation, rounded on its own, so the result has one bit pattern.  NO LISTED TARGET IS
 * SKIPPED, a zero weight included: 0 * inf and 0 * NaN are NaN, as IEEE 754 says, and a rest component of -0.0 becomes +0.0 where a
 * zero-weight target lists the vertex (-0.0 + 0.0 is +0.0) and stays -0.0 where none does.  Weights are used as given: any sign, above
 * 1, denormal; nothing is clamped or normalised.  A dense target lists every vertex.  If the call also gives bones for the mesh, m --
 * not the rest vertex -- then goes through exactly PT_DEFORM_BONES' arithmetic (pt_deform.h) with the rig pt_scene_bind_skin bound: the
 * result is that skinning of the morphed vertices, bit for bit.  Nothing compounds: every call starts from REST, whatever a previous
 * morph or deform left; and a later PT_DEFORM_BONES still skins the rest vertices, not the morphed ones.  ALL INSTANCES OF A MESH SHARE
 * ITS SHAPE: two faces with different expressions are two meshes.
 *
 * Memory, on top of pt_deform.h: a bound set is 4 bytes per vertex (the rows' starts) and 16 bytes per listed (vertex, delta) pair
 * (dx, dy, dz, target); a call keeps one weight table of 4 bytes per target of its meshes.  A morphed mesh uses the two vertex buffers of
 * pt_deform.h, allocated by its first morph or deform and reused by every later one: the morphed vertex of a call with bones stays in
 * registers, there is no third buffer.
 *
 *   - pt_scene_bind_morphs: binds a set to one mesh.  Everything is checked on the host before any device work, EVERY VERTEX INDEX
 *     INCLUDED: no index >= n_vertices ever reaches the device, and the kernel checks none.  The lists are then turned vertex-major on the
 *     host, once -- a stable counting sort by vertex, so that a vertex's entries stand in ascending target order -- and uploaded once.  A
 *     mesh has one set, a new one replaces it.  n_targets == 0 or targets == NULL unbinds.  Binding changes no geometry.
 *     PT_ERR_INVALID: a null scene or set; a target with n_deltas > 0 and null deltas; vertex indices that are not strictly ascending;
 *     a vertex index >= n_vertices; a dense target whose n_deltas is not n_vertices; a mesh index out of range or a mesh no instance uses;
 *     a scene with a live pt_frame, as for a pose.  PT_ERR_UNSUPPORTED: a scene without instances; more than 2^31 - 1 entries in one set.
 *     The call holds the scene's render lock.
 *   - pt_scene_morph does three things in order.
 *     1. Every mesh named in morphs[n_morphs] gets current vertices by the arithmetic above from weights[n_weights], and with
 *        bones != NULL from bones[n_bones][12], rows 0 .. 2 of every bone's mat4.  One kernel launch per morphed mesh on the scene's
 *        stream, no host wait before the assembly.  A mesh named more than once takes its last entry.
 *     2. The instances named by `instances` get transforms[n][16] exactly as by pt_scene_pose; n == 0: the pose stays.
 *     3. What a pose does: ONE batched assembly over all instances and the tree rebuilt aside, adopted only when it is complete.
 *     After the call the scene is, through every entry point (those pt_pose.h lists), bit for bit the scene a fresh
 *     pt_scene_create_meshes gives for meshes whose vertices are what pt_scene_get_mesh_vertices returns, as after pt_scene_deform.  A
 *     call that fails leaves the scene AND the current vertices of every mesh as they were.
 *     PT_ERR_INVALID: a null scene; null morphs with n_morphs > 0; null weights; a mesh index out of range or a mesh no instance uses;
 *     a mesh without a bound set; n_weights other than the set's target count; bones for a mesh without a bound skin, or n_bones other
 *     than the skin's bone count; and, word for word as for pt_scene_pose: null transforms with n > 0; an index >= the instance count;
 *     instances == NULL with another n than 0 or the instance count; a scene with a live pt_frame.  PT_ERR_UNSUPPORTED: a scene without
 *     instances.  All of these before any device work.  The call holds the scene's render lock.  `info` (may be NULL) receives what the
 *     call did.
 *   - pt_scene_get_morphs: the target count of the set bound to `mesh` and the (vertex, delta) pairs it lists (0 and 0 for none); either
 *     pointer may be NULL.  PT_ERR_INVALID: a null scene, a mesh out of range or unused.  PT_ERR_UNSUPPORTED: a scene without instances.
 *
 * OUT OF SCOPE: motion vectors of a morphed mesh (made, as for a deformed one, by the marked calls of pt_motion_shapes.h); weights per instance; morphed normals as an input
 * of their own (the assembler computes normals from the vertices); building the vertex-major rows on the device. */
#ifndef PT_MORPH_ABI_H
#define PT_MORPH_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_morph_target { /* one target of a set */
    uint32_t n_deltas;      /* listed vertices (dense: n_vertices); 0: an empty target */
    const uint32_t *vertex; /* [n_deltas], strictly ascending, each < n_vertices; NULL: dense, entry i is vertex i */
    const float *delta;     /* [n_deltas][3] */
} pt_morph_target;

typedef struct pt_morph_set {       /* the targets bound to one mesh of the scene */
    uint32_t mesh;                  /* mesh index of the creating pt_scene_create_meshes call */
    uint32_t n_targets;             /* >= 1 (0: unbind) */
    const pt_morph_target *targets; /* [n_targets] (NULL: unbind) */
} pt_morph_set;

typedef struct pt_mesh_morph { /* one mesh's weights, and its pose of bones */
    uint32_t mesh;
    const float *weights;  /* [n_weights], used as given */
    uint32_t n_weights;    /* must be the set's target count, else PT_ERR_INVALID */
    const float *bones;    /* [n_bones][12], rows 0..2 of each bone's mat4, or NULL: the morph alone */
    uint32_t n_bones;      /* with bones: must be the bound skin's bone count */
} pt_mesh_morph;

typedef struct pt_morph_info {
    uint32_t n_instances, n_triangles; /* the fields of pt_deform_info, with their meanings ... */
    uint32_t assembly_syncs;
    uint32_t assembly_chunks;
    float upload_ms, assembly_ms, tree_ms, rest_ms, total_ms;
    uint32_t n_meshes_deformed;        /* (meshes morphed; a mesh named twice counts once) */
    uint32_t n_vertices_skinned;       /* (vertices of the meshes morphed with bones) */
    float skin_ms;                     /* (0: the skinning is part of the morph kernel, in morph_ms) */
    float vertex_upload_ms;            /* (wall clock of the uploads of weights and bone tables) */
    uint32_t allocations;
    uint32_t n_vertices_morphed;       /* ... vertices the morph kernel made */
    float morph_ms;                    /* device events around the morph launches */
    uint64_t n_entries_read;           /* (vertex, delta) pairs of the sets of the morphed meshes */
} pt_morph_info;

int pt_scene_bind_morphs(pt_scene *scene, const pt_morph_set *set);
int pt_scene_morph(pt_scene *scene, const pt_mesh_morph *morphs, uint32_t n_morphs, const uint32_t *instances, uint32_t n,
                   const float *transforms /* [n][16], rows */, pt_morph_info *info /* may be NULL */);
int pt_scene_get_morphs(pt_scene *scene, uint32_t mesh, uint32_t *n_targets, uint64_t *n_entries);

#ifdef __cplusplus
}
#endif

#endif
