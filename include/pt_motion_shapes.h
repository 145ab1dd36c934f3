/* pt_motion_shapes.h -- motion for deformed meshes: the scene remembers what it looked like at the previous frame, and the feature pass
 * reprojects per vertex.  Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h includes this file behind
 * pt_motion.h and pt_deform.h, which it needs; it is not meant to be included on its own.
 *
 * pt_render_features_motion (pt_motion.h) describes an instance by its matrix alone.  A mesh that pt_scene_deform or pt_scene_morph bent
 * between two frames has no such description: where a surface point was before depends on its face.  The entry points here let the scene
 * itself keep "the previous frame" -- a MARK -- and describe a hit on a deformed mesh through the three vertices of its face as they were
 * at the mark.
 *
 *   - pt_scene_motion_mark records the previous frame: the current instance matrices (host memory) and, per used mesh, its shape.  A mesh
 *     at its rest vertices is marked by their address (rest vertices never change: nothing is copied).  A deformed mesh's current vertices
 *     are copied device to device, on the scene's stream, into a buffer of the mesh's own: 12 bytes per vertex, allocated by the mesh's
 *     first such mark, reused by every later one and counted in pt_deform_info::allocations.  Every mesh has a shape serial that every
 *     successful pt_scene_deform / pt_scene_morph bumps for the meshes it names; the mark stores the serials.  A new mark replaces the
 *     old one.  The first mark turns TRACKING on: from then on every successful rebuild (pose, deform, morph) also produces, for every
 *     instance triangle t (counted from the first instance triangle), face_of[t]: the scene-wide number of the face it came from -- the
 *     faces of all instances end to end in instance order, before any is rejected.  4 bytes per face of all instances, twice (the table
 *     of a rebuild is made aside and swapped in at adoption; a failed call keeps the old one), allocated by the first mark and counted
 *     likewise; one more kernel launch per assembly chunk (pt_face_table_kernel), no host wait.
 *     The call holds the scene's render lock, as a pose does, and is allowed with a live pt_frame: it changes no geometry and no render.
 *     PT_ERR_INVALID: a null scene.  PT_ERR_UNSUPPORTED: a scene without instances.  Both before any device work.  A mark whose
 *     allocations fail leaves the previous mark as it was; one whose device copies fail leaves the scene WITHOUT a mark (the copies
 *     overwrite the buffers the previous mark names).
 *   - pt_scene_motion_unmark frees all of that and turns tracking off: the scene then takes exactly the path it took before it was
 *     marked, allocates nothing new and launches nothing new.  Without a mark it does nothing.  Refusals as for the mark.
 *   - pt_scene_get_motion_mark: the marked matrices [n_instances][16] and the kind [n_instances] a marked features call would give every
 *     instance now (either may be NULL).  Decided on the host, with C = the instance's current matrix and P = its marked one:
 *       the instance's mesh has the marked serial: pt_motion_table's kind for (C, P): PT_MOTION_STATIC, PT_MOTION_MOVED or PT_MOTION_NONE;
 *       the serial differs and every entry of P is finite: PT_MOTION_DEFORMED (the serial decides, not the values: a mesh deformed back
 *       to equal vertices is still DEFORMED);
 *       the serial differs and an entry of P is not finite: PT_MOTION_NONE.
 *     PT_ERR_INVALID: a null scene, a scene without a mark.  PT_ERR_UNSUPPORTED: a scene without instances.
 *   - pt_scene_get_triangle_faces: downloads face_of: out[instance triangles] (may be NULL: the number alone), *n (may be NULL) their
 *     number.  PT_ERR_INVALID without a mark, and -- with the message "no rebuild since the first mark" -- when nothing was rebuilt since
 *     tracking began: there is no table yet, and none is made for the question (a features call never needs it in that state, because no
 *     instance can be DEFORMED).
 *   - pt_render_features_motion_marked[_device]: pt_render_features_motion[_device] with the mark as the previous frame.  out_features is
 *     pt_render_features' result bit for bit; out_motion has pt_render_features_motion's format, so pt_temporal_denoise_motion[_device]
 *     takes it unchanged.  When no instance is DEFORMED the call IS pt_render_features_motion with the marked matrices (same launch, same
 *     bits) and reads no face table.  Otherwise (pt_motion_shapes_kernel) STATIC, MOVED and NONE instances are described exactly as
 *     there, and a ray that hits triangle record (a, ab, ac) of object obj of a DEFORMED instance at pos with shading normal n gets:
 *       g = face_of[obj - first instance object],  k = g - the instance's first face,  (ia, ib, ic) = faces[3k ..] of its mesh
 *       Qa, Qb, Qc: the marked vertices ia, ib, ic through the marked matrix M with the assembler's arithmetic: for the four rows r
 *           d = 0; d += M[r][0]*x; d += M[r][1]*y; d += M[r][2]*z; d += M[r][3]*1.0f   -> h[r];   Q = h[0..2] * (1.0f / h[3])
 *         which makes them, bit for bit, the corners the assembler made of that face at the marked frame
 *       barycentrics as the shading normal's: ap = pos - a; d00 = ab.ab, d01 = ab.ac, d11 = ac.ac, d20 = ap.ab, d21 = ap.ac (each dot
 *           from zero, in index order); inv = 1 / (d00*d11 - d01*d01); v = (d11*d20 - d01*d21) * inv; w = (d00*d21 - d01*d20) * inv;
 *           u = 1 - v - w
 *       pp = (Qa*u + Qb*v) + Qc*w
 *       c' = cross(Qb - Qa, Qc - Qa), l' = (c'.x c'.x + c'.y c'.y) + c'.z c'.z;   c = cross(ab, ac), l likewise
 *       !(l' > 0), !(l > 0) or a component of pp that is not finite: the ray has NO PREVIOUS POSITION: pp = pn = 0, moved 1, none 1
 *         (a face that was degenerate at the mark and survives now, for one)
 *       otherwise ng' = c' * (1/sqrtf(l')), ng = c * (1/sqrtf(l)), v = (n - ng) + ng',
 *           pn = v * (1/sqrtf((v.x v.x + v.y v.y) + v.z v.z)) if that sum is > 0, else 0;  moved 1, none 0
 *     THE PREVIOUS NORMAL IS AN APPROXIMATION: the current shading normal carried by the change of the face normal.  It is exact where
 *     the shading normal is the face normal (flat instances) and first-order for smooth ones; the temporal push only tests it against a
 *     tolerance (normal_min).  The previous position is exact up to the rounding of the barycentrics.
 *     Refusals: pt_render_features_motion's, and PT_ERR_INVALID for a scene without a mark (PT_ERR_UNSUPPORTED without instances) -- all
 *     before any device work.
 *
 * Left out: view batches, followed features (pt_features.h), motion blur, previous SMOOTH normals (see above), and marks older than one
 * frame: a scene has one mark. */
#ifndef PT_MOTION_SHAPES_ABI_H
#define PT_MOTION_SHAPES_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

enum { PT_MOTION_DEFORMED = 3 };

typedef struct pt_motion_mark_info {
    uint32_t n_instances;
    uint32_t n_meshes_copied;   /* deformed meshes whose current vertices were copied */
    uint64_t bytes_copied;
    uint32_t allocations;       /* as pt_deform_info::allocations, this call's included */
    float total_ms;             /* wall clock, the copies waited for */
} pt_motion_mark_info;

int pt_scene_motion_mark(pt_scene *scene, pt_motion_mark_info *info /* may be NULL */);
int pt_scene_motion_unmark(pt_scene *scene);
int pt_scene_get_motion_mark(pt_scene *scene, float *out_transforms /* [n_instances][16] */, uint8_t *out_kind /* [n_instances] */);
int pt_scene_get_triangle_faces(pt_scene *scene, uint32_t *out /* [instance triangles] */, uint32_t *n);
int pt_render_features_motion_marked(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, float *out_features /* [H][W][3][4] */,
                                     float *out_motion /* [H][W][2][4] */);
int pt_render_features_motion_marked_device(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, float *d_out_features, float *d_out_motion,
                                            void *stream);

#ifdef __cplusplus
}
#endif

#endif
