// PathTrace/temporal_denoise.h -- temporal denoising of the frames of a sequence (a camera path, a turntable, processViews' output): an
// extension of PathTrace/denoise.h.
#ifndef PATHTRACE_TEMPORAL_DENOISE_H
#define PATHTRACE_TEMPORAL_DENOISE_H

#include <PathTrace/camera.h>
#include <PathTrace/denoise.h>
#include <PathTrace/image/image.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

#include <vector>

// pt_temporal_params of pt_hip.h: the spatial filter of every frame, and the temporal step in front of it.
struct TemporalDenoiseParams {
    DenoiseParams spatial;                  // pt_denoise's filter, as denoise() applies it
    float alpha_color = 0.2F;               // lower bound of the colour's blend weight, (0, 1]
    float alpha_moments = 0.2F;             // ... of the luminance moments', (0, 1]
    int max_history = 32;                   // history length cap, >= 1
    int moments_min_history = 4;            // history length from which the luminance variance is temporal, >= 1
    float sigma_luminance_temporal = 4.0F;  // luminance sigma where it is
    float normal_min = 0.9F;                // least dot product of the normals of a reprojected tap
    float position_tolerance = 2.0F;        // largest distance of a reprojected tap, in pixel footprints
    // reproject through the poses and the shapes of the scene's mesh instances (Scene::pose, deform, morph between the pushes;
    // include/pt_motion.h and pt_motion_shapes.h)
    bool follow_motion = false;
};

// The temporal half of SVGF in front of denoise()'s spatial filter: every push reprojects the history of the frames pushed before it
// (through the pixels' first-hit positions) and blends it into the new frame before filtering.  By default the history is reprojected as
// for a Scene that does not move.  With params.follow_motion every push ends by marking the scene (pt_scene_motion_mark on its first
// replica: the instances' matrices and every mesh's shape) and the next one reprojects where each pixel's surface was at that mark
// (pt_render_features_motion_marked, pt_temporal_denoise_motion): through the matrices for a Scene that was only posed in between -- the
// result a previous-pose table gives, bit for bit --, per vertex for meshes that Scene::deform or Scene::morph changed.  The first push,
// and the first after reset(), have no previous frame; a Scene whose number of instances changed, or whose mark was taken away
// (Scene::unmarkMotion), resets the history.  The scene stays marked when the object goes (Scene::unmarkMotion frees it).  The first push,
// and the first after reset(), equals denoise() with params.spatial bit for bit.  One device history per object, on the scene's first
// replica; the scene must outlive the object.  Throws std::invalid_argument for parameters outside their range or a frame of another
// size than options.image_width x image_height, std::runtime_error if the device fails.
class TemporalDenoiser {
  public:
    TemporalDenoiser(const Scene &scene, const RenderOptions &options, const TemporalDenoiseParams &params = {});
    ~TemporalDenoiser();
    TemporalDenoiser(const TemporalDenoiser &) = delete;
    TemporalDenoiser &operator=(const TemporalDenoiser &) = delete;

    // denoises `frame`, rendered through `camera`: renders the camera's features and pushes them with the frame
    Image<> push(const Image<> &frame, const Camera &camera);
    // forgets the history: the next push has none
    void reset();

  private:
    const Scene &scene;
    RenderOptions options;
    struct pt_temporal *handle = nullptr;
    bool follow_motion = false;
    bool has_pose = false;         // follow_motion: the push before left its mark on the scene
    std::vector<float> last_pose;  // [instances][16]: its size is the instance count of that push
};

// frames[v] seen through cameras[v], pushed in order through one TemporalDenoiser.
std::vector<Image<>> denoiseSequence(const std::vector<Image<>> &frames, const Scene &scene, const std::vector<const Camera *> &cameras,
                                     const RenderOptions &options, const TemporalDenoiseParams &params = {});

#endif
