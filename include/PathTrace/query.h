// PathTrace/query.h -- scene queries of the C++ API: what a pixel of a frame shows, and whether a segment is blocked (Scene::pick,
// Scene::occluded, declared in PathTrace/detail/world.h; the C ABI is include/pt_query.h, which has the definitions).  Not part of the
// reference's API: an editor that lets its user click on a preview needs the instance and the face under the cursor.
#ifndef PATHTRACE_QUERY_H
#define PATHTRACE_QUERY_H

#include <PathTrace/base.h>
#include <PathTrace/camera.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

#include <cstdint>

struct PickResult {
    static constexpr uint32_t no_face = 0xFFFFFFFFu;
    bool hit = false;
    float t = -1.0F;
    const Object *object = nullptr;  // as Scene::getIntersection reports it: valid until the next pose, deform, morph or relight for a mesh triangle
    int32_t object_index = -1;       // construction order: the constructor's objects, then the mesh instances' surviving triangles
    int32_t instance = -1;           // the mesh instance the triangle belongs to, or -1
    uint32_t face = no_face;         // the face of the instance's MeshData, where known (include/pt_query.h), else no_face
    vec3<float> position{0.0F, 0.0F, 0.0F};
    vec3<float> normal{0.0F, 0.0F, 0.0F};           // shading normal (getSurfaceNormal)
    vec3<float> geometric_normal{0.0F, 0.0F, 0.0F}; // of the triangle's winding, not turned towards the ray; a sphere's is its normal
    float b1 = 0.0F, b2 = 0.0F;      // weights of the triangle's 2nd and 3rd corner; 0 for a sphere
};

#endif
