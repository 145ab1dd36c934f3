// PathTrace/gather.h -- light gathered at surface points of the C++ API: ambient occlusion, direct light or whole paths at points, at a
// frame's first hits and at the corners of a mesh instance's triangles (Scene::gather, Scene::gatherFrame, Scene::bakeInstance, declared
// in PathTrace/detail/world.h; the C ABI is include/pt_gather.h, which has the definitions).  Not part of the reference's API: getSample is
// reachable there only through Camera::shootRay, and a baker or an irradiance probe holds a position and a normal, not a camera.
#ifndef PATHTRACE_GATHER_H
#define PATHTRACE_GATHER_H

#include <PathTrace/base.h>
#include <PathTrace/camera.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

#include <array>
#include <cstdint>
#include <limits>
#include <vector>

enum class GatherKind : int32_t {
    occlusion = 0, // the share of cosine-distributed rays that meet nothing within `distance`
    direct = 1,    // the light samples of one vertex: a white Lambertian receiver's direct light
    paths = 2,     // whole paths from the point: getSample behind a first vertex that is already there
};

struct GatherOptions {
    GatherKind kind = GatherKind::occlusion;
    int samples = 16;
    float epsilon = 1E-3F;
    float distance = std::numeric_limits<float>::infinity(); // occlusion only
    uint64_t base_seed = 0;                                    // sample s of point i draws from RandomEngine(pt_pixel_seed(base_seed, s, i))
};

struct GatherPoint {
    vec3<float> position{0.0F, 0.0F, 0.0F};
    vec3<float> normal{0.0F, 1.0F, 0.0F}; // unit length
};

struct GatherResult {
    Color<float> value{};  // rgb: the mean over the samples (occlusion: the unoccluded share in all three); alpha 1
    uint32_t samples = 0;  // 0: a frame's pixel whose ray hits nothing
    uint32_t occluded = 0; // occlusion: the occluded samples
};

#endif
