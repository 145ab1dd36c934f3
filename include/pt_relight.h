/* pt_relight.h -- a new look for a scene in place: materials, point lights and the material of mesh instances.  Part of
 * the C ABI of libpathtrace_hip.so: include/pt_hip.h includes this file behind pt_motion.h; it is not meant to be included on its own.
 *
 * The feature serves the scenes that keep their description: those of pt_scene_create_meshes with at least one instance (what pt_pose.h
 * lists as kept).  Every other scene gets PT_ERR_UNSUPPORTED from all three entry points, as from pt_scene_pose: a plain pt_scene_create
 * scene keeps neither its description nor its triangles' exact vertices, and making such scenes editable is a separate decision about
 * memory (36 bytes per triangle).  On top of what pt_pose.h lists, a scene with instances keeps the depth-first order of its leaves in
 * device memory: 4 bytes per object -- the device builder's array, no longer freed, or the host builder's order uploaded by the first
 * relight -- and, behind the first relight, the table of the description's objects (4 bytes per object of the description).
 *
 *   - pt_scene_relight: replaces the look of the scene.
 *       materials != NULL: the material table is replaced whole by materials[n_materials] (n_materials may be 0 with a non-NULL pointer).
 *       The description's own triangles and spheres keep their material INDEX: their look changes by editing their table entry.
 *       set_point_lights != 0: the point lights are replaced by light_pos[n][3] / light_spectrum[n][4]; n may be 0.
 *       instances / instance_material [n_instance_materials]: instance instances[k] gets the material instance_material[k] (an index or
 *       PT_NO_MATERIAL); an index that occurs more than once gets the last of its materials.
 *     Nothing of this touches the tree, the leaf records' geometry or the normals: the material table and the light table are uploaded,
 *     the material word of every triangle of an instance that changes is rewritten, and the emitter registry with its CDF
 *     (Scene::registerEmissiveObjects, reference src/scene/scene.cpp:167-208) is rebuilt by one ordered pass on the device over the
 *     depth-first leaf order.  After the call the scene is, through every entry point, bit for bit the scene a fresh
 *     pt_scene_create_meshes gives for the same geometry with the new look.  It keeps its address, its stream and its render workspace.
 *     A later pt_scene_pose keeps the new look.
 *     Short cut: when no instance changes material, the number of lights is unchanged and every material's emission is bit-equal to
 *     before, the registry stays and only the tables are uploaded (info->registry_rebuilt = 0).
 *     PT_ERR_INVALID, before any device work, the scene as it was: a null scene or look; a null array with a non-zero count; an unknown
 *     BSDF kind; an instance index >= the instance count; a material index in use after the call (description triangles, spheres,
 *     instances) that is neither PT_NO_MATERIAL nor < the new n_materials; a scene with a live pt_frame (destroy the frames first).
 *     PT_ERR_UNSUPPORTED: a scene without instances (before any device work); more than 32 light samples per path vertex with the new
 *     look (point lights + emitter samples) -- the count is only known once the registry exists, so everything new is built aside and
 *     adopted only when complete: the scene is as it was then, too.
 *     The call holds the scene's render lock.  A TemporalDenoiser that holds history of this scene is not reset: the radiance changed,
 *     the geometry did not; pt_temporal_reset is advised after a large edit, the caller decides.
 *   - pt_scene_get_materials / pt_scene_get_point_lights: the current tables.  The count goes to *n_materials / *n_point_lights (may be
 *     NULL); at most `capacity` entries are written (the out pointers may be NULL when capacity is 0). */
#ifndef PT_RELIGHT_ABI_H
#define PT_RELIGHT_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_relight {
    const pt_material *materials; uint32_t n_materials;   /* NULL: the table stays; else it is replaced whole */
    int32_t set_point_lights;                             /* 0: the lights stay */
    const float *light_pos, *light_spectrum; uint32_t n_point_lights;   /* [n][3], [n][4]; n may be 0 */
    const uint32_t *instances, *instance_material; uint32_t n_instance_materials; /* instance k gets material[k] or PT_NO_MATERIAL; a repeated index gets the last */
} pt_relight;
typedef struct pt_relight_info {
    uint32_t n_emissive, n_object_samples, n_candidates;  /* after the call; candidates = objects with a lit material (0 when the registry stayed) */
    uint32_t registry_rebuilt, triangles_rewritten;       /* 0/1; triangles whose material word was rewritten */
    float registry_ms, total_ms;                          /* device events / wall clock */
} pt_relight_info;

int pt_scene_relight(pt_scene *scene, const pt_relight *look, pt_relight_info *info /* may be NULL */);
int pt_scene_get_materials(const pt_scene *scene, pt_material *out, uint32_t capacity, uint32_t *n_materials);
int pt_scene_get_point_lights(const pt_scene *scene, float *out_pos, float *out_spectrum, uint32_t capacity, uint32_t *n_point_lights);

#ifdef __cplusplus
}
#endif

#endif
