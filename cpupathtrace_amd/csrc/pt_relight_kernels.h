// pt_relight_kernels.h -- the device side of pt_scene_relight (pt_relight.hip): the emitter registry of a scene by one
// ordered pass over the depth-first order of its leaves, and the material word of the triangles of mesh instances.
#ifndef PT_RELIGHT_KERNELS_H
#define PT_RELIGHT_KERNELS_H

#include <hip/hip_runtime.h>

#include <cstdint>

// What the registry pass reads of a scene with mesh instances (all device memory)
struct PtRelightScene {
    const uint32_t *order = nullptr;    // [n_objects] object indices, leaves depth-first left to right (Scene::registerEmissiveObjects order)
    uint32_t n_objects = 0;
    const uint32_t *desc_ref = nullptr; // [n_desc_objects] triangle index, or PT_REF_SPHERE | sphere index, of every object of the description
    uint32_t n_desc_objects = 0, n_desc_tris = 0; // object n_desc_objects + k is triangle n_desc_tris + k
    const float4 *recs = nullptr;       // leaf records, PT_TRI_QUADS per triangle: [2].y material, [2].z object | cull << 31 (pt_types.h)
    const float4 *spheres = nullptr;    // [n_spheres] origin, radius
    const uint2 *sph_meta = nullptr;    // [n_spheres] material, object
    const float *tri_pos = nullptr;     // [n_triangles][9] the triangles' exact vertices
    const float4 *materials = nullptr;  // [n_materials][4] the table of the new look
    uint32_t n_materials = 0;
};

// Positions per workgroup of the pass, and the workgroups for n positions
constexpr uint32_t PT_RELIGHT_BLOCK = 256;
inline uint32_t pt_relight_blocks(uint32_t n) {
    return (n + PT_RELIGHT_BLOCK - 1) / PT_RELIGHT_BLOCK;
}

// Step 1 of 2.  For every position of the order whether its object registers as an emitter (power > 0 and power * area > 0, the host's
// arithmetic operation for operation): one ballot word per 64 positions to ballots[ceil(n / 64)], the number of survivors before every
// workgroup (an exclusive scan) to block_first[pt_relight_blocks(n)], and to counts[0] the number of survivors, to counts[1] the number
// of candidates (objects whose material has power > 0).  counts needs no clearing.
hipError_t pt_relight_flag(hipStream_t stream, const PtRelightScene &scene, unsigned long long *ballots, uint32_t *block_first, uint32_t *counts);

// Step 2 of 2.  The survivors compacted in the order's order: survivor k's four-quad record to emis[4 * k] (the layout of create_scene:
// vertices or sphere, reference, cull flag, material index, emission), its probability power * area to prob[k] and its object to obj[k].
// The arrays hold counts[0] entries.
hipError_t pt_relight_emit(hipStream_t stream, const PtRelightScene &scene, const unsigned long long *ballots, const uint32_t *block_first, float4 *emis, float *prob,
                           uint32_t *obj);

// One range of triangles that get one material
struct PtRelightRange {
    uint32_t first_tri, count, material, pad;
};
// The material word of every triangle of the ranges (device memory, n_ranges of them, `total` triangles in all, none empty, sorted by
// first_tri and disjoint), in the leaf records and in the shading records; nothing else is written.
hipError_t pt_relight_materials(hipStream_t stream, const PtRelightRange *ranges, uint32_t n_ranges, uint32_t total, float4 *recs, float4 *tri_shade);

#endif
