// PathTrace/radiance.h -- radiance along free rays and captures of the C++ API: the mean radiance that arrives along rays the caller
// chooses, and whole images of such rays made on the device by an equirectangular, cube-map, fisheye or orthographic camera model
// (Scene::radiance, Scene::capture, declared in PathTrace/detail/world.h; the C ABI is include/pt_radiance.h, which has the definitions).
// Not part of the reference's API: the only camera there is Camera, and getSample is reachable only through it.
#ifndef PATHTRACE_RADIANCE_H
#define PATHTRACE_RADIANCE_H

#include <PathTrace/base.h>
#include <PathTrace/image/image.h>
#include <PathTrace/scene/scene.h>

#include <cstdint>
#include <vector>

struct RadianceOptions {
    int samples = 64;
    float epsilon = 1E-3F;
    uint64_t base_seed = 0; // sample s of ray or pixel i draws from RandomEngine(pt_pixel_seed(base_seed, s, i))
};

struct RadianceResult {
    Color<float> value{};  // the mean over the samples; alpha: the share of samples whose first walk hit something
    uint32_t samples = 0;  // the samples taken
    uint32_t missed = 0;   // samples whose first walk hits nothing
    uint32_t outside = 0;  // samples without a ray (a fisheye's pixels outside the image circle)
};

enum class CaptureModel : int32_t {
    equirect = 0, // a 360 x 180 degree panorama: row 0 looks along up, the image centre along forward
    cube = 1,     // six square faces side by side (+right, -right, +up, -up, +forward, -forward): width == 6 * height
    fisheye = 2,  // equidistant, `fov` across the image circle: width == height
    ortho = 3,    // parallel rays along forward through a window of 2 * extent
};

// The basis is used as given: never normalised, never re-orthogonalised.  lookAt makes an orthonormal one.
struct Capture {
    CaptureModel model = CaptureModel::equirect;
    int width = 0;
    int height = 0;
    bool jitter = true; // a jittered position per sample; false: pixel centres
    vec3<float> origin{0.0F, 0.0F, 0.0F};
    vec3<float> right{-1.0F, 0.0F, 0.0F};
    vec3<float> up{0.0F, 1.0F, 0.0F};
    vec3<float> forward{0.0F, 0.0F, 1.0F};
    float fov = 3.14159274101257324219F; // fisheye: the full angle across the image circle, radians, 0 < fov <= 2 pi
    float extent_x = 1.0F;               // ortho: half the width and half the height of the window, scene units
    float extent_y = 1.0F;

    // forward = normalize(look_at - origin), right = normalize(cross(forward, up)), up re-made from the two
    void lookAt(vec3<float> from, vec3<float> look_at, vec3<float> up_hint) {
        origin = from;
        forward = (look_at - from).normalize();
        right = cross(forward, up_hint).normalize();
        up = cross(right, forward);
    }
};

#endif
