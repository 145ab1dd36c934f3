/* pt_query.h -- scene queries: what a ray, a pixel or every pixel of a frame hits, and whether a segment is blocked.
 * Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h includes this file at its end; it is not meant to be included on its own.
 *
 * One 64-byte pt_hit per query.  The walk is pt_intersect_batch's (pt_closest_kernel's, unchanged), so `t` and `object` are its answers
 * bit for bit; everything else is derived once per query, after the walk, from what the scene already holds on the device:
 *
 *   t, object   pt_intersect_batch's out_t and out_obj.  A MISS is t = -1, object = -1, instance = -1, face = PT_QUERY_NO_FACE, material =
 *               PT_NO_MATERIAL and 0 in every other float.
 *   instance    the mesh instance whose object range (pt_scene_instance_ranges) holds `object`; -1 for an object of the description and
 *               in a scene without instances.
 *   face        the face of the instance's mesh the hit triangle came from, where that is known:
 *                 (a) the instance kept every face of its mesh (its object count equals the mesh's face count): the assembler keeps
 *                     faces in face order, so the face is the triangle's index inside the instance, object - first object;
 *                 (b) the scene has a face table (pt_scene_get_triangle_faces would succeed: a motion mark and a rebuild since):
 *                     face = face_of[object - first instance object] - the scene-wide number of the instance's face 0.
 *               Where both apply they agree.  Otherwise -- and for spheres and the description's triangles -- PT_QUERY_NO_FACE.  No table
 *               is built for the question: a caller who needs the faces of meshes that lose faces to the assembler marks the scene
 *               (pt_scene_motion_mark) and poses it once.
 *   position    o + d * t, each component one product and one sum.
 *   material    the index the hit object carries (PT_NO_MATERIAL as it is).
 *   normal      the shading normal (Triangle / Sphere::getSurfaceNormal: what the path kernel shades with), not turned towards the ray.
 *   b1, b2      triangle (a, ab, ac): the weights of the 2nd and 3rd corner, with the arithmetic include/pt_motion_shapes.h states for its
 *               barycentrics: ap = position - a; d00 = ab.ab, d01 = ab.ac, d11 = ac.ac, d20 = ap.ab, d21 = ap.ac (each dot summed from
 *               zero in index order); inv = 1 / (d00*d11 - d01*d01); b1 = (d11*d20 - d01*d21) * inv; b2 = (d00*d21 - d01*d20) * inv.
 *               (1 - b1 - b2) * a + b1 * b + b2 * c is the position up to rounding.  Sphere: 0, 0.
 *   geometric_normal  triangle: c * (1/sqrtf(l)) with c = cross(ab, ac), l = (c.x c.x + c.y c.y) + c.z c.z; 0 where !(l > 0).  NOT turned
 *               towards the ray: its side is the triangle's winding.  Sphere: the shading normal.
 *
 * Entry points.  The host forms take host memory and return when the results are there.  The _device forms take DEVICE pointers for
 * queries and results and a hipStream_t: the work is ordered behind what that stream holds and the stream's later work behind it, as
 * pt_render_features_device does; a null stream makes the call wait.
 *   - pt_query_rays: n rays (origin xyz, direction xyz).
 *   - pt_query_pixels: the ray through the CENTRE of pixel (x, y) of the frame options describes: the camera ray of pt_render_features
 *     with a sub-pixel offset of 0, no aperture and no jitter -- a pure function of camera and pixel.  The host form refuses a pixel
 *     outside the frame (PT_ERR_INVALID) before any device work; the device form cannot look, and answers for the ray through
 *     that pixel's centre all the same (the formula has a value for every integer pair).
 *   - pt_query_frame: the same for every pixel, out[y * image_width + x]: the ID and attribute map of a frame.
 *   - pt_occluded_rays: n segments (origin xyz, direction xyz, t_max).  out[i] = 1 iff the closest hit of (origin, direction) has
 *     0 <= t < t_max, else 0: t_max = +inf asks "is there anything at all", a NaN or negative t_max gives 0.  The walk is the path
 *     kernel's shadow walk: it ends at the first hit below t_max it meets, and is NOT pruned at t_max (pruning there is not the same
 *     thing in floating point), so the answer is exactly the definition's.
 * Refusals, all before any device work: a null argument (n == 0 needs no arrays), more than 0x7fffffff queries, an image size that is
 * not positive: PT_ERR_INVALID.  n == 0 is PT_OK without a launch.  Every call holds the scene's render lock, changes nothing in the scene,
 * and is allowed with a live pt_frame and with or without a motion mark.
 *
 * Left out: a minimum distance (the reference has none), instance visibility masks, view batches of ID maps, building a face table
 * without a mark. */
#ifndef PT_QUERY_ABI_H
#define PT_QUERY_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

#define PT_QUERY_NO_FACE 0xFFFFFFFFu

typedef struct pt_hit {
    float t; int32_t object; int32_t instance; uint32_t face;
    float position[3]; uint32_t material;
    float normal[3]; float b1;
    float geometric_normal[3]; float b2;
} pt_hit;

int pt_query_rays(pt_scene *scene, const float *rays /* [n][6] */, size_t n, pt_hit *out /* [n] */);
int pt_query_rays_device(pt_scene *scene, const float *d_rays, size_t n, pt_hit *d_out, void *stream);
int pt_query_pixels(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const int32_t *xy /* [n][2] */, size_t n, pt_hit *out /* [n] */);
int pt_query_pixels_device(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const int32_t *d_xy, size_t n, pt_hit *d_out, void *stream);
int pt_query_frame(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, pt_hit *out /* [H][W] */);
int pt_query_frame_device(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, pt_hit *d_out, void *stream);
int pt_occluded_rays(pt_scene *scene, const float *segments /* [n][7]: origin, direction, t_max */, size_t n, uint8_t *out /* [n] */);
int pt_occluded_rays_device(pt_scene *scene, const float *d_segments, size_t n, uint8_t *d_out, void *stream);

#ifdef __cplusplus
}
#endif

/* The nearest surface to a free point and distance grids (pt_nearest_points, pt_distance_grid_fill): they report
 * instance and face by this file's rules, and are declared, with their contracts, in: */
#include "pt_nearest.h"

#endif
