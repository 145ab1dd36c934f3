// PathTrace/light_probes.h -- light probes of the C++ API: the radiance that arrives at free points from every direction as spherical
// harmonics of bands 0..2, grids of such probes, and the lookup that shades a point with a normal from a grid (Scene::lightProbes,
// Scene::lightProbeGrid, Scene::shadeWithLightProbes, declared in PathTrace/detail/world.h; the C ABI is include/pt_light_probes.h, which
// has the definitions).  Not part of the reference's API: an irradiance volume for a moving object holds positions, not cameras.
#ifndef PATHTRACE_LIGHT_PROBES_H
#define PATHTRACE_LIGHT_PROBES_H

#include <PathTrace/base.h>
#include <PathTrace/gather.h>
#include <PathTrace/scene/scene.h>

#include <array>
#include <cstdint>
#include <vector>

struct LightProbeOptions {
    int samples = 256;
    float epsilon = 1E-3F;
    uint64_t base_seed = 0;       // sample s of probe i draws from RandomEngine(pt_pixel_seed(base_seed, s, i))
    float max_backfacing = 0.25F; // the lookup leaves out a probe that sees more than this share of its samples from behind
};

struct LightProbe {
    std::array<std::array<float, 3>, 9> sh{}; // sh[k][c]: coefficient k (bands 0..2) of colour channel c
    uint32_t samples = 0;
    uint32_t missed = 0;     // samples whose ray hits nothing
    uint32_t backfacing = 0; // samples that see their first surface from behind
};

struct LightProbeGrid {
    vec3<float> origin{0.0F, 0.0F, 0.0F};
    vec3<float> step{1.0F, 1.0F, 1.0F};
    std::array<uint32_t, 3> count{1, 1, 1}; // probe (ix, iy, iz) has index (iz * ny + iy) * nx + ix
};

#endif
