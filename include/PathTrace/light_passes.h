// PathTrace/light_passes.h -- light-group passes of the C++ API: the radiance of Scene::radiance's rays and Scene::capture's pixels split by
// the emitter group a term came from and, optionally, by bounce depth, and the mix that turns such passes back into an image under new
// gains -- trace once, then turn lights up, down or to another colour for nothing (Scene::lightPasses, Scene::captureLightPasses, declared
// in PathTrace/detail/world.h, and mixLightPasses below; the C ABI is include/pt_light_passes.h, which has the definitions).
// Not part of the reference's API.
#ifndef PATHTRACE_LIGHT_PASSES_H
#define PATHTRACE_LIGHT_PASSES_H

#include <PathTrace/base.h>
#include <PathTrace/radiance.h>

#include <array>
#include <cstdint>
#include <vector>

enum class LightPassComponent : int32_t {
    emitted = 0,  // the light source seen along the ray itself
    direct = 1,   // one scattering: the light samples at the first vertex, and the emission a bounce ray finds at the second
    indirect = 2, // everything else
};

// The group (0 .. n_groups - 1) of every material of the device scene's table and of every point light, the lights in the order the Scene
// was given them.  A Scene gives every distinct MaterialHandler one slot of the table, in the order in which it first meets them -- the
// objects in their order, then the mesh instances --; pt_scene_get_materials(scene.deviceScene(), ...) returns the table and its count.
// The lengths must be the scene's current counts: a table made before a relight that changed them is refused behind it.
struct LightGroups {
    uint32_t n_groups = 1;                  // 1..8
    bool split = false;                     // three passes per group (emitted, direct, indirect) instead of one
    std::vector<uint8_t> material_group;    // [materials of the scene]
    std::vector<uint8_t> point_light_group; // [point lights of the scene]

    size_t passes() const { return static_cast<size_t>(n_groups) * (split ? 3U : 1U); }
    size_t pass(uint32_t group, LightPassComponent component = LightPassComponent::emitted) const {
        return split ? 3U * group + static_cast<size_t>(component) : group;
    }
};

// The passes of n rays, or of the width * height pixels of a capture in row order: pass p of ray or pixel i is value[i * n_passes + p]
// (rgb).  total: Scene::radiance's or Scene::capture's record of each, bit for bit, or empty where it was not asked for.  The passes of a
// ray add up to its total only nearly: the same terms are added in another order.
struct LightPasses {
    size_t n_passes = 0;
    int width = 0, height = 0; // of a capture; 0 for rays
    std::vector<std::array<float, 3>> value;
    std::vector<RadianceResult> total;

    size_t size() const { return n_passes == 0 ? 0 : value.size() / n_passes; }
    const std::array<float, 3> &at(size_t i, size_t pass) const { return value[i * n_passes + pass]; }
};

// out[i] = the passes of ray or pixel i weighed by gains[pass] (rgb) and added in pass order, in fp32, every product rounded before it is
// added; alpha: total's where passes.total is there, else 0.  gains.size() must be passes.n_passes.  Computed on the host.
std::vector<Color<float>> mixLightPasses(const LightPasses &passes, const std::vector<std::array<float, 3>> &gains);

#endif
