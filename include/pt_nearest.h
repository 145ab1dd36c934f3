/* pt_nearest.h -- nearest-surface queries: the closest point of the scene's surfaces to a free point, and unsigned distance grids
 * (DESIGN.md 4.24).  Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h reaches this file at its end, through the last line of
 * pt_query.h, whose instance and face rules it shares; it is not meant to be included on its own.
 *
 * One 64-byte pt_nearest per query (p, r): p = xyz, r = max_distance.
 *
 * THE DEFINITION.  A minimum over all objects: it depends neither on the tree nor on the order of a traversal.
 *   - r2 = r * r, one fp32 product.  Every object k has a squared distance d2_k from the arithmetic below.  The answer is the object with
 *     the smallest d2_k among those with d2_k <= r2.  Ties in the bits of d2 go to the lowest leaf-record index: triangle t (the t-th
 *     triangle in object order) has index t, sphere i (the i-th sphere in object order) has index n_triangles + 1 + i.
 *   - An object whose d2 is NaN is never the answer.
 *   - A MISS: no object in range, a NaN or negative r, a NaN coordinate of p, an empty scene.  A miss has distance = squared_distance =
 *     +inf, object = instance = -1, face = PT_QUERY_NO_FACE, material = PT_NO_MATERIAL and every other word 0.
 *   - r = +inf means unbounded.  (An infinite coordinate of p is not special: every d2 is then +inf or NaN, so the query is a miss
 *     whenever r2 is finite.)
 *
 * All arithmetic is fp32, every operation on its own (no fused multiply-add); every dot product is summed from zero in index order.
 *
 * Triangle (a, ab, ac) of the leaf record (ab = b - a, ac = c - a as the scene formed them):
 *     ap = p - a;   d1 = ab.ap;  d2 = ac.ap
 *     bp = ap - ab; d3 = ab.bp;  d4 = ac.bp
 *     cp = ap - ac; d5 = ab.cp;  d6 = ac.cp
 *     vc = d1*d4 - d3*d2;  vb = d5*d2 - d1*d6;  va = d3*d6 - d5*d4
 *   The regions are tested in this order and the first that holds decides (v, w, feature):
 *     1  d1 <= 0 && d2 <= 0                                  v = 0            w = 0              feature 4 (vertex a)
 *     2  d3 >= 0 && d4 <= d3                                 v = 1            w = 0              feature 5 (vertex b)
 *     3  vc <= 0 && d1 >= 0 && d3 <= 0                       v = d1/(d1-d3)   w = 0              feature 1 (edge ab)
 *     4  d6 >= 0 && d5 <= d6                                 v = 0            w = 1              feature 6 (vertex c)
 *     5  vb <= 0 && d2 >= 0 && d6 <= 0                       v = 0            w = d2/(d2-d6)     feature 3 (edge ca)
 *     6  e1 = d4-d3, e2 = d5-d6: va <= 0 && e1 >= 0 && e2 >= 0   v = 1 - w    w = e1/(e1+e2)     feature 2 (edge bc)
 *     7  otherwise, den = 1/((va+vb)+vc)                     v = vb*den       w = vc*den         feature 0 (face)
 *   diff = (ap - ab*v) - ac*w per component;  squared_distance = diff.diff;  distance = sqrtf(squared_distance), correctly rounded;
 *   position = (a + ab*v) + ac*w;  b1 = v, b2 = w (the weights of the 2nd and 3rd corner);  geometric_normal is pt_hit's (include/
 *   pt_query.h);  side = the sign of diff . cross(ab, ac): +1, -1, or 0 for zero or NaN.
 *
 * Sphere (c, R):
 *     pc = p - c;  len = sqrtf(pc.pc);  dist = fabsf(len - R);  squared_distance = dist*dist;  distance = dist
 *     position = c + pc * (R / len), and c + (R, 0, 0) where len == 0
 *     geometric_normal = pc * (1/len), and (1, 0, 0) where len == 0
 *     side = +1, -1 or 0 for len above, below or equal to R (0 for NaN);  feature = 7;  b1 = b2 = 0
 *
 * object, instance, face and material are found as pt_hit's are (include/pt_query.h: the instance whose object range holds the object,
 * the face by its two rules).
 *
 * THE GRID.  Cell (ix, iy, iz), at index (iz*ny + iy)*nx + ix, is the query at origin[a] + (float)i_a * step[a] -- one product and one
 * sum per axis, the position rule of pt_light_probes_grid -- with r = max_distance.  The positions are made on the device.  out_distance
 * is that query's distance (unsigned, +inf on a miss), out_object its object (-1 on a miss); out_object may be NULL.
 *
 * Entry points.  The host forms take host memory and return when the results are there.  The _device forms take DEVICE pointers and a
 * hipStream_t: the work is ordered behind what that stream holds and the stream's later work behind it, as pt_query_rays_device's is; a
 * null stream makes the call wait.
 * Refusals, all before any device work: a null argument (n == 0 needs no arrays; out_object may be null), more than 0x7fffffff queries
 * or cells, a zero count: PT_ERR_INVALID.  n == 0 is PT_OK without a launch.
 * Every call holds the scene's render lock, changes nothing in the scene, and is allowed beside a live pt_frame and with or without a
 * motion mark.
 *
 * Left out: a robust inside/outside test -- `side` is the side of ONE primitive, and an angle-weighted pseudo-normal would need mesh
 * adjacency the scene does not keep --, the k nearest objects, queries restricted to one instance, and signed grids. */
#ifndef PT_NEAREST_ABI_H
#define PT_NEAREST_ABI_H

#ifdef __cplusplus
extern "C" {
#endif

#define PT_NEAREST_FACE 0u
#define PT_NEAREST_EDGE_AB 1u
#define PT_NEAREST_EDGE_BC 2u
#define PT_NEAREST_EDGE_CA 3u
#define PT_NEAREST_VERTEX_A 4u
#define PT_NEAREST_VERTEX_B 5u
#define PT_NEAREST_VERTEX_C 6u
#define PT_NEAREST_SPHERE 7u

typedef struct pt_nearest {            /* 64 bytes, four 16-byte stores */
    float distance; int32_t object; int32_t instance; uint32_t face;
    float position[3]; uint32_t material;
    float geometric_normal[3]; float b1;
    float squared_distance; uint32_t feature; int32_t side; float b2;
} pt_nearest;

typedef struct pt_distance_grid { float origin[3]; float step[3]; uint32_t count[3]; } pt_distance_grid; /* cell (ix,iy,iz) at (iz*ny+iy)*nx+ix */

int pt_nearest_points(pt_scene *scene, const float *points /* [n][4]: xyz, max_distance */, size_t n, pt_nearest *out /* [n] */);
int pt_nearest_points_device(pt_scene *scene, const float *d_points, size_t n, pt_nearest *d_out, void *stream);
int pt_distance_grid_fill(pt_scene *scene, const pt_distance_grid *grid, float max_distance, float *out_distance /* [nz][ny][nx] */,
                          int32_t *out_object /* same shape, may be NULL */);
int pt_distance_grid_fill_device(pt_scene *scene, const pt_distance_grid *grid, float max_distance, float *d_out_distance, int32_t *d_out_object, void *stream);

#ifdef __cplusplus
}
#endif

#endif
