// PathTrace/nearest.h -- nearest-surface queries of the C++ API: the closest point of the scene's surfaces to free points, and unsigned
// distance grids (Scene::nearest, Scene::distanceGrid, declared in PathTrace/detail/world.h; the C ABI is include/pt_nearest.h, which
// has the definition).  Not part of the reference's API: a tool that places probes, snaps points to a mesh, tests clearance or bakes a
// distance field asks where the nearest surface is, not what a ray hits.
#ifndef PATHTRACE_NEAREST_H
#define PATHTRACE_NEAREST_H

#include <PathTrace/base.h>
#include <PathTrace/scene/scene.h>

#include <array>
#include <cstdint>
#include <limits>
#include <vector>

enum class NearestFeature : uint32_t { face = 0, edge_ab = 1, edge_bc = 2, edge_ca = 3, vertex_a = 4, vertex_b = 5, vertex_c = 6, sphere = 7 };

struct NearestResult {
    static constexpr uint32_t no_face = 0xFFFFFFFFu;
    bool found = false;              // false: nothing within max_distance (or a NaN point or distance): everything below is as it stands here
    float distance = std::numeric_limits<float>::infinity();
    float squared_distance = std::numeric_limits<float>::infinity(); // what the objects were compared by
    const Object *object = nullptr;  // as Scene::getIntersection reports it: valid until the next pose, deform, morph or relight for a mesh triangle
    int32_t object_index = -1;       // construction order: the constructor's objects, then the mesh instances' surviving triangles
    int32_t instance = -1;           // the mesh instance the triangle belongs to, or -1
    uint32_t face = no_face;         // the face of the instance's MeshData, where known (include/pt_query.h), else no_face
    vec3<float> position{0.0F, 0.0F, 0.0F};         // the closest point
    vec3<float> geometric_normal{0.0F, 0.0F, 0.0F}; // of the triangle's winding; a sphere's is its normal towards the query
    float b1 = 0.0F, b2 = 0.0F;      // weights of the triangle's 2nd and 3rd corner at the closest point; 0 for a sphere
    NearestFeature feature = NearestFeature::face;
    int side = 0;                    // of THIS primitive: +1 in front of the winding / outside the sphere, -1 behind / inside, 0 on it
};

struct DistanceGrid {
    vec3<float> origin{0.0F, 0.0F, 0.0F};
    vec3<float> step{1.0F, 1.0F, 1.0F};
    std::array<uint32_t, 3> count{1, 1, 1}; // cell (ix, iy, iz) has index (iz * ny + iy) * nx + ix
};

struct DistanceField {
    std::vector<float> distance;  // unsigned; +inf where nothing lies within max_distance
    std::vector<int32_t> object;  // the nearest object's index, -1 there
};

#endif
