/*
 * pt_hip.h -- C ABI of libpathtrace_hip.so, the MI355X (gfx950) implementation of CPUPathTrace's hot path.
 *
 * The reference has no FFI layer: its boundary for this path is the C++ API of include/PathTrace/worker.h and
 * include/PathTrace/scene/scene.h (all citations are file:line under the reference tree).  Each entry point below names
 * the reference interface it replaces; INTEGRATION.md shows the binding a maintainer adds on the reference side.
 * Plain C types only: pointers + sizes in, status code out (0 = PT_OK); pt_last_error() describes the last failure of the
 * calling thread.  The caller owns every host buffer; the library owns device memory behind the opaque pt_scene handle.
 * There is no CPU fallback: without a usable HIP device every compute entry point fails with PT_ERR_NO_DEVICE.
 */
#ifndef PT_HIP_H
#define PT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OK 0
#define PT_ERR_INVALID 1     /* bad argument (null pointer, negative size, index out of range) */
#define PT_ERR_NO_DEVICE 2   /* no HIP device / device index out of range */
#define PT_ERR_HIP 3         /* a HIP runtime call failed */
#define PT_ERR_UNSUPPORTED 4 /* scene outside what the kernels cover (see pt_scene_create) */
#define PT_ERR_NOMEM 5
#define PT_ERR_CANCELLED 6   /* a controlled render stopped early (budget or pt_render_cancel): see pt_render_tiles_ctl */

enum { PT_OBJ_TRIANGLE = 0, PT_OBJ_SPHERE = 1 };
enum { PT_BSDF_LAMBERTIAN = 0, PT_BSDF_GLASS = 1, PT_BSDF_MIRROR = 2 };
enum { PT_APERTURE_NONE = 0, PT_APERTURE_CIRCULAR = 1, PT_APERTURE_HEXAGONAL = 2 };
#define PT_NO_MATERIAL 0xFFFFFFFFu /* object keeps the default handler: white Lambertian (src/scene/object.cpp:9-11,32) */

/* ConstantMaterial + BSDF behind one ConstantMaterialHandler (scene/material.h:53-68, scene/propagation.h:58-108,
 * scene/object.h:26-40).  specular is Material::getSpecularColor (white unless a subclass overrides it). */
typedef struct pt_material {
    float diffuse[4];
    float specular[4];
    float emission[4];
    float ior;
    int32_t bsdf;    /* PT_BSDF_* */
    int32_t one_way; /* MirrorBRDF(one_way) */
    int32_t pad;
} pt_material;

/* The std::vector<std::unique_ptr<Object>> and std::vector<std::unique_ptr<LightSource>> handed to Scene::Scene
 * (scene/scene.h:32), flattened.  Objects keep their construction order: obj_kind[i] tells whether object i is the next
 * entry of the triangle arrays or of the sphere arrays.  Object indices reported by pt_intersect_batch are positions in
 * this order. */
typedef struct pt_scene_desc {
    uint32_t n_objects;
    const uint8_t *obj_kind;      /* [n_objects] PT_OBJ_* */
    uint32_t n_triangles;
    const float *tri_pos;         /* [n_triangles][9] a, b, c                  (scene/object.h:126-128) */
    const float *tri_nrm;         /* [n_triangles][9] normal_a, _b, _c; NULL = face normals (object.cpp:118-124) */
    const uint8_t *tri_cull;      /* [n_triangles] cull_backface              (scene/object.h:134) */
    const uint32_t *tri_material; /* [n_triangles] index into materials or PT_NO_MATERIAL */
    uint32_t n_spheres;
    const float *sph;             /* [n_spheres][4] origin xyz, radius        (scene/object.h:101-103) */
    const uint32_t *sph_material; /* [n_spheres] */
    uint32_t n_materials;
    const pt_material *materials;
    uint32_t n_point_lights;
    const float *light_pos;       /* [n_point_lights][3] PointLightSource::pos      (scene/light.h:55) */
    const float *light_spectrum;  /* [n_point_lights][4] PointLightSource::spectrum (scene/light.h:56) */
} pt_scene_desc;

/* Arguments of Camera::Camera (camera.h:92,108-109). */
typedef struct pt_camera_params {
    float origin[3];
    float look_at[3];
    float up[3];
    float focal_length;
    float height;
    float aspect_ratio;
    float aperture_width;
    float aperture_height;
    int32_t aperture_kind; /* PT_APERTURE_* : nullptr / CircularApertureSampler / HexagonalApertureSampler(hex_ratio) */
    float hex_ratio;
    float focal_plane_dist;
} pt_camera_params;

/* RenderOptions (worker.h:14-31).  allow_bias is never read by the reference and has no field here: a caller who allows bias denoises the
 * finished frame with pt_render_features + pt_denoise (below), as the C++ processJob does. */
typedef struct pt_options {
    int32_t image_width;
    int32_t image_height;
    int32_t min_sample_count;
    int32_t max_sample_count;
    float epsilon;
} pt_options;

/* WorkItem (worker.h:44-62). */
typedef struct pt_tile {
    int32_t x, y, w, h;
} pt_tile;

/* One processItem(WorkItem(job, x, y, w, h), engine) call (worker.h:69): the pixels of the rectangle are rendered in row-major
 * order through ONE engine whose raw xorshift state is rng_state on entry (base.h:24-38). */
typedef struct pt_stream {
    int32_t x, y, w, h;
    uint64_t rng_state;
} pt_stream;

/* Work done by one render call, counted on the device by the kernel itself; the time is measured with HIP events around the launch
 * on the library's stream. */
typedef struct pt_stats {
    uint64_t samples;           /* getSample calls (worker.cpp:194) */
    uint64_t rays_traced;       /* closest-hit + shadow rays walked through the tree */
    uint64_t shadow_rays_traced;
    uint64_t node_visits;       /* inner nodes visited = pairs of AABB slab tests */
    uint64_t leaf_tests;        /* Triangle/Sphere::getIntersection calls */
    uint64_t vertices;          /* path vertices shaded */
    uint64_t launches;          /* launches of the path kernel (one per render call) */
    double kernel_ms;           /* duration of the launch */
    uint64_t wave_steps;        /* traversal steps executed by wavefronts (each serves up to 64 walks) */
    uint64_t shading_passes;    /* shading passes executed by wavefronts */
    uint64_t wavefronts;        /* wavefronts of the launch */
    uint64_t slot_rows;         /* rows of 64 stream slots per wavefront */
} pt_stats;

typedef struct pt_scene pt_scene;

/* Number of usable HIP devices (0 when there is none or the runtime cannot be initialised). */
int pt_device_count(void);

const char *pt_last_error(void);

/* Scene::Scene (src/scene/scene.cpp:153-181): builds the reference's BVH topology (impl::constructBVH, scene.cpp:12-102) -- on
 * the device, level by level (pt_build.hip), for scenes of PT_BUILD_DEVICE_MIN (1024) objects and more, by the same recursion on the host
 * for smaller ones; the two produce the same tree bit for bit -- registers emissive objects (scene.cpp:183-208) and lays everything out
 * in device arrays on `device`.
 * PT_ERR_UNSUPPORTED: more than 32 light samples per path vertex (point lights + min(2 + log10(E + 1), E) object samples: Scene::sampleLights
 * itself has no bound, scene.cpp:226,231; 32 are the bits of this library's per-vertex visibility mask),
 * or a BVH deeper than 128 levels.
 * Thread safety: calls on DIFFERENT scenes may run concurrently; render and intersection calls on the SAME scene are serialised inside
 * the library (one workspace per scene), so callers that run processItem from several threads on one Scene -- as the reference's
 * doWork does (src/worker.cpp:328-362) -- are correct, they just do not overlap on the device. */
int pt_scene_create(int device, const pt_scene_desc *desc, pt_scene **out);
void pt_scene_destroy(pt_scene *scene);

/* Introspection for tests: node count of the reference-topology BVH (2 * n_objects - 1), its depth, emissive object count. */
int pt_scene_info(const pt_scene *scene, uint64_t *n_nodes, uint32_t *depth, uint32_t *n_emissive);
/* Emissive objects in Scene::registerEmissiveObjects order (scene.cpp:183-208) with their normalised cumulative selection
 * probabilities (scene.cpp:167-180); at most `capacity` entries are written, the count is returned in *n_written. */
int pt_scene_emissive(const pt_scene *scene, int32_t *out_obj, float *out_cdf, uint64_t capacity, uint64_t *n_written);
/* Pre-order dump of the BVH: out_obj[i] = object index of a leaf or -1 for an inner node, out_box[i] = low xyz, high xyz. */
int pt_scene_bvh_dump(const pt_scene *scene, int32_t *out_obj, float *out_box, uint64_t capacity, uint64_t *n_written);

/* Scene::getIntersection (scene/scene.h:41, src/scene/scene.cpp:210-220) for n rays (origin xyz, direction xyz each).
 * out_t < 0 means miss (then out_obj = -1); otherwise out_obj is the construction-order index of the closest object. */
int pt_intersect_batch(pt_scene *scene, const float *rays, size_t n, float *out_t, int32_t *out_obj);

/* processItem (worker.h:69, src/worker.cpp:149-326) for n independent streams, all in flight at once on the device.
 * out_image is the full row-major image (image_width * image_height * 4 floats, index (y * width + x) * 4 as image/image.h:80-89);
 * only pixels covered by a stream are written.  out_states[i] (may be NULL) receives stream i's engine state afterwards. */
int pt_render_streams(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const pt_stream *streams, size_t n,
                      float *out_image, uint64_t *out_states, pt_stats *stats);

/* processItem for ONE WorkItem, returning only the item's rectangle: out_tile is item->w * item->h * 4 floats, row-major inside the
 * rectangle (the Image<> processItem returns, worker.h:69); *out_state (may be NULL) receives the engine state afterwards.  The frame the
 * item belongs to never exists on the host. */
int pt_render_item(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const pt_stream *item, float *out_tile,
                   uint64_t *out_state, pt_stats *stats);

/* processJob (worker.h:83-84, src/worker.cpp:389-424) restricted to the given tiles: every pixel is its own 1x1 stream whose
 * engine is RandomEngine(pt_pixel_seed(base_seed, x, y)) -- the reference seeds its workers from std::random_device
 * (worker.cpp:369-382), so any seeding conforms; this one makes the image independent of tiling and of the GPU count. */
int pt_render_tiles(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles,
                    uint64_t base_seed, float *out_image, pt_stats *stats);

/* Same, reporting progress the way processJob's progress_callback does (worker.h:75-84, src/worker.cpp:354-360): `progress(completed,
 * total, user)` is called from the CALLING thread, never concurrently, with completed = 1 .. n_tiles in increasing order, while the
 * device is still rendering (the kernel counts finished tiles in host-visible memory; the host polls).  NULL = no reporting.
 * The callback runs while the library holds the scene's render lock: it must not call back into the library with the same scene (a
 * preview through processItem would wait for itself), and it must not throw through this C interface (src/host/worker.cpp keeps a
 * C++ callback's exception and throws it again after the call). */
typedef void (*pt_progress_fn)(int completed, int total, void *user);
int pt_render_tiles_progress(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles,
                             uint64_t base_seed, float *out_image, pt_stats *stats, pt_progress_fn progress, void *user);

/* processJob on several devices of one node -- the multi-device form of doWorkParallel (src/worker.cpp:364-387).  scenes[i] are replicas of
 * one scene created on different devices (pt_scene_create(device_i, same desc)); the tiles are dealt round-robin to the scenes (tile k to
 * scenes[k % n_scenes]; along the diagonals of the tile grid when its rows hold a multiple of n_scenes tiles, so that no device renders
 * whole columns of the frame), one host thread per scene, and only the rectangles of a device's own tiles are copied into out_image.
 * The image is identical for every n_scenes (per-pixel engines).  stats, if not NULL, is an array of n_scenes entries.  progress as in
 * pt_render_tiles_progress, counted over all devices and never concurrent -- but with n_scenes > 1 it is called from the library's
 * worker threads (as the reference calls it from its worker threads, worker.h:75-78), not from the calling thread.
 * MEASURED ONLY WITH REPLICAS ON ONE DEVICE so far (tests): no multi-GPU node was available to the build. */
int pt_render_tiles_multi(pt_scene *const *scenes, int n_scenes, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles,
                          size_t n_tiles, uint64_t base_seed, float *out_image, pt_stats *stats, pt_progress_fn progress, void *user);

/* Same, writing into DEVICE memory (e.g. a torch tensor's data_ptr) and ordered on `stream` (a hipStream_t, NULL = the
 * library's own stream followed by a synchronisation).  Used for the multi-GPU gather over RCCL.  Does not wait for the device unless
 * `stats` is given; every waiting entry point checks that the launch rendered all its streams, this one with stats or PT_VERIFY=1. */
int pt_render_tiles_device(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles,
                           uint64_t base_seed, float *d_out_image, void *stream, pt_stats *stats);

/* processJob for n_views cameras of one scene in one launch per replica (a turntable, a camera path, a stereo pair: small frames that one
 * at a time leave most of the device idle).  Every view is options->image_width x image_height, tiled as pt_job_tiles; view v's pixels are
 * seeded from (base_seeds[v], x, y) and equal pt_render_tiles(camera = cameras[v], base_seed = base_seeds[v]) bit for bit; one view is
 * that call.  out_images: [n_views][height][width][4] floats.  The views' tiles are dealt to the replicas as in pt_render_tiles_multi;
 * progress counts the tiles of all views (n_views * pt_job_tiles(width, height)).  PT_ERR_INVALID without a launch for n_views <= 0, null
 * tables, or more than 0x0fffffff pixels in all.  The views share the options.  The resumable form of a batch is pt_frame_create_views
 * (below); one pt_frame_render call of such a frame with a `ctl` is the controlled render of a batch, at the frame path's overhead
 * (+5.8 % on the metric frame). */
int pt_render_views(pt_scene *const *scenes, int n_scenes, const pt_camera_params *cameras, const uint64_t *base_seeds, int32_t n_views,
                    const pt_options *options, float *out_images, pt_stats *stats, pt_progress_fn progress, void *user);
/* Same, one scene, into DEVICE memory (e.g. a [V, H, W, 4] torch tensor's data_ptr), ordered on `stream` as pt_render_tiles_device. */
int pt_render_views_device(pt_scene *scene, const pt_camera_params *cameras, const uint64_t *base_seeds, int32_t n_views,
                           const pt_options *options, float *d_out_images, void *stream, pt_stats *stats);

/* Cancellable, time-budgeted processJob.  A controlled render is the same single launch per replica as pt_render_tiles_multi; it can be
 * told to stop while it runs, either by pt_render_cancel (from the progress callback or any other thread) or by its budget.
 *   - The stop is COOPERATIVE.  The host writes a word in pinned host memory; every wavefront of the launch reads it once per shading pass.
 *     From then on no stream (pixel) is taken any more, and a stream that would start another sample is dropped at that sample boundary.
 *     The launch then ends on its own.  It takes roughly one path's bounces plus the longest walk in flight (DESIGN.md reports drain_ms).
 *     It is no watchdog: a walk that never ends never reaches a sample boundary.
 *   - Pixels: a pixel is written only when its estimator finishes, so every written pixel is bit-identical to the full render's.  Every
 *     other pixel keeps the value out_image held on entry (a pre-filled sentinel shows which is which).  tile_done says which tiles finished.
 *   - Status: PT_OK = every tile finished, even if a stop came too late to drop anything; PT_ERR_CANCELLED = stopped, some tiles unfinished;
 *     any other code = failure, as for pt_render_tiles_multi.  The launch must account for every stream
 *     (finished + abandoned + unclaimed = pixels of the tiles); if it does not, the call fails with PT_ERR_HIP.
 *   - The scenes are fully reusable afterwards: their next render of any kind equals a fresh scene's, bit for bit.
 * scenes, n_scenes, tiles, progress: as pt_render_tiles_multi (stats, if not NULL, has n_scenes entries for what did run).  `cancel` is
 * only ever set by pt_render_cancel; it is not cleared by a call, so a control that was cancelled before a call stops that call at once. */
typedef struct pt_render_control {
    double budget_ms;           /* in: wall-clock budget counted from the call's start; <= 0 = none */
    uint8_t *tile_done;         /* in: [n_tiles] or NULL; out: tile_done[i] = 1 if every pixel of tiles[i] finished, else 0 */
    uint64_t streams_finished;  /* out: streams (pixels) that finished */
    uint64_t streams_abandoned; /* out: taken, then dropped at a sample boundary */
    uint64_t streams_unclaimed; /* out: never taken */
    double drain_ms;            /* out: from the stop request to the end of the launch(es), as the host saw it; 0 if no stop was requested */
    int32_t cancel;             /* set by pt_render_cancel only */
} pt_render_control;
int pt_render_tiles_ctl(pt_scene *const *scenes, int n_scenes, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles,
                        size_t n_tiles, uint64_t base_seed, float *out_image, pt_stats *stats, pt_progress_fn progress, void *user,
                        pt_render_control *ctl);
/* Requests the stop of the controlled render that runs (or will run) with `ctl`.  Thread-safe and non-blocking; it may be called from the
 * progress callback or any other thread.  PT_ERR_INVALID for NULL. */
int pt_render_cancel(pt_render_control *ctl);

/* A resumable frame: a controlled render that can be continued.  pt_frame_create fixes a job (scenes, camera, options, tiles, seed) and
 * launches nothing; every pt_frame_render continues it -- one launch per replica that still has work -- until the frame is complete.  A
 * stop (budget or pt_render_cancel) drops every stream at its next sample boundary as in pt_render_tiles_ctl, but a stream that has taken
 * samples PARKS there: its engine state, pixel, estimator and closed candidates go to the frame's park storage in HBM, and the next call
 * resumes it from them.  Pixels are seeded per pixel from (base_seed, x, y), so the finished frame is bit-identical to one uninterrupted
 * pt_render_tiles_multi / pt_render_tiles_ctl call with the same arguments, however it was sliced.
 *   - pt_frame_create copies camera, options and tiles, and deals the tiles to the replicas as pt_render_tiles_multi does, for good.
 *   - pt_frame_render: PT_OK = the frame is complete (a complete frame returns PT_OK at once, without a launch); PT_ERR_CANCELLED =
 *     stopped again.  Pass the same out_image every time: a pixel is written by the call that finishes it and never again; the others keep
 *     the caller's values.  ctl (may be NULL: run the rest of the frame to completion) is used as by pt_render_tiles_ctl, except that
 *     tile_done ([n_tiles] of the frame) reports the whole frame's tiles, streams_abandoned counts the streams this call parked, and
 *     streams_unclaimed the streams it left to start afresh (never taken, or dropped before their first sample).  progress reports
 *     (completed, total) over the whole frame, strictly increasing from call to call.  stats: n_scenes entries, zero for replicas that did not launch.
 *   - Scenes must outlive their frames.  Several frames may share a scene and their calls may be interleaved with each other and with
 *     any other render on the scene, in any order: each frame owns its park storage, and the scene's calls are serialised as always.
 *   - A failure (any code but PT_OK and PT_ERR_CANCELLED) leaves the frame failed: every later call returns the same code.
 *   - Park storage: two buffers per replica of min(streams left, slots of the launch) records of 528 bytes.
 * pt_render_tiles_ctl and every other entry point are unchanged: they never park. */
typedef struct pt_frame pt_frame;
typedef struct pt_frame_info {
    uint64_t streams_total;          /* pixels of the frame's tiles */
    uint64_t streams_finished;
    uint64_t streams_parked;         /* dropped with samples taken: resumed from their park record by the next call */
    uint64_t streams_untouched;      /* to start afresh from their seed */
    uint64_t tiles_total;
    uint64_t tiles_done;
    uint64_t samples_carried;        /* samples the parked streams have taken of their current pixel */
    uint64_t parked_with_candidates; /* parked streams whose estimator holds closed candidates */
    uint64_t park_bytes;             /* device memory of the park storage, all replicas */
    int32_t launches;                /* launches made so far, all replicas */
    int32_t status;                  /* PT_OK, or the code that failed the frame */
} pt_frame_info;
int pt_frame_create(pt_scene *const *scenes, int n_scenes, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles,
                    size_t n_tiles, uint64_t base_seed, pt_frame **out);
/* A resumable frame over a view batch: the job of pt_render_views (same arguments, same tile list -- pt_job_tiles(width, height) of every view,
 * moved down by v * height, dealt to the replicas as always), behind the same handle.  pt_frame_render, pt_frame_get_info, pt_frame_preview and
 * pt_frame_destroy work on it with the contracts above; out_image / image / out_rgba are [n_views][height][width][4], out_samples is
 * [n_views][height][width], tile_done and progress cover n_views * pt_job_tiles(width, height) tiles.  However the calls were sliced, the
 * finished image equals pt_render_views with the same arguments bit for bit (so view v equals pt_render_tiles(cameras[v], base_seeds[v])).
 * The frame keeps its own copies of the cameras and seeds, on the host and in device tables of its own: other batches on the same scenes
 * between two slices do not disturb it.  n_views == 1 is pt_frame_create over pt_job_tiles(width, height) with base_seeds[0].
 * PT_ERR_INVALID before anything is uploaded: n_views <= 0, null tables, more than 0x0fffffff pixels or more than 2^31 - 1 rows in all;
 * PT_ERR_NO_DEVICE as pt_frame_create.
 * Preview of a view frame: per view as described at pt_frame_preview; with `denoise` the features are pt_render_features_views with the frame's
 * cameras and the filter is the view form of the masked filter, so a hole is filled only from taps of its own view.  One device keeps about
 * 2^20 streams in flight: a batch of more pixels than that has whole views that are still holes after its first slice (the work list is
 * view after view) -- unless the frame is progressive (pt_frame_set_progressive): then every view has its samples after every pass. */
int pt_frame_create_views(pt_scene *const *scenes, int n_scenes, const pt_camera_params *cameras, const uint64_t *base_seeds, int32_t n_views,
                          const pt_options *options, pt_frame **out);
int pt_frame_render(pt_frame *frame, float *out_image, pt_stats *stats, pt_progress_fn progress, void *user, pt_render_control *ctl);
/* Progressive mode of a resumable frame: the frame is rendered in PASSES, and after pass k every unfinished pixel of the
 * frame has taken exactly target_k = target_(k-1) + quantum samples (target_0 = 0) -- the whole picture refines together, however many
 * pixels the frame has.  In a pass every unfinished stream is taken once, samples its pixel until the pixel has the target (or its
 * estimator finishes it first, as always), parks and gives its slot to the next stream of the pass; one pass is one launch per replica.
 * The finished frame is bit-identical to pt_render_tiles / pt_render_views with the same arguments for every quantum, every change of the
 * quantum between calls and every placement of stops: each pixel still runs its own engine through the same chain of samples.
 *   - pt_frame_set_progressive: quantum >= 1 turns the mode on or changes the step of the passes to come (a pass in progress keeps its
 *     target); 0 turns it off: the frame goes on as a plain resumable frame from the records it has.  max_passes_per_call <= 0 = no limit.
 *     Only between two pt_frame_render calls (it takes the frame's lock).  PT_ERR_INVALID for a null frame or a negative quantum; a
 *     failed frame returns its code.  A stream that already has the target's samples when the mode is turned on (a frame sliced before)
 *     takes none in that pass.
 *   - pt_frame_render on a progressive frame runs pass after pass until the frame is complete (PT_OK), the budget or pt_render_cancel
 *     stops it (PT_ERR_CANCELLED, as always), or max_passes_per_call passes have COMPLETED in this call and work is left
 *     (PT_ERR_CANCELLED as well: stopped, call again).  A pass that a stop cut short is finished by the next call before a new one
 *     starts, its streams below the target first.  No sample is ever lost: a stream the stopped launch did not reach keeps its record.
 *     stats sum the call's launches (launches, kernel_ms and the work counters); ctl's streams_finished counts all of them,
 *     streams_abandoned and streams_unclaimed describe the call's last pass.  Progress, tile_done, replicas and view frames as always.
 *   - Park storage of a progressive frame: two buffers per replica of one record per stream left (528 bytes each; 2 x 1.1 GB for
 *     1920 x 1080), allocated by its first passes and reported by pt_frame_get_info's park_bytes.
 *   - pt_frame_preview between two passes has no holes inside the frame's tiles: every unfinished pixel shows its running mean. */
int pt_frame_set_progressive(pt_frame *frame, int32_t quantum, int32_t max_passes_per_call);
typedef struct pt_frame_progress {
    int32_t quantum, max_passes_per_call;
    int32_t passes_completed;
    int32_t target;                 /* of the pass in progress or last completed */
    int32_t pass_in_progress;       /* 1 = a stop cut the last pass short */
    int32_t min_samples, max_samples; /* samples taken, over unfinished pixels (0, 0 when there is none) */
    uint64_t streams_at_target;     /* unfinished streams with at least `target` samples, after a progressive pass */
    uint64_t samples_lost;          /* always 0: a progressive frame that dropped a record would fail instead */
} pt_frame_progress;
int pt_frame_get_progress(const pt_frame *frame, pt_frame_progress *out);
/* (the info of a frame: `pt_frame_info` names the struct, so the function is pt_frame_get_info) */
int pt_frame_get_info(const pt_frame *frame, pt_frame_info *info);
int pt_frame_destroy(pt_frame *frame);
/* The noise of a frame and its noise target: every unfinished pixel rated by the standard error of its mean, a summary and a map of the
 * ratings, and a progressive frame that holds the pixels at or below a target and stops once enough of them are.  The
 * struct pt_frame_noise and the two entry points that take it and set the target are declared, with their contracts, in: */
#include "pt_frame_noise.h"

/* The tile list processJob builds (worker.cpp:398-414): tile_size = clamp(min(w, h) / 4, 1, 32), row-major, edge tiles clipped.
 * Returns the tile count; fills at most `capacity` entries. */
size_t pt_job_tiles(int32_t image_width, int32_t image_height, pt_tile *out, size_t capacity);

uint64_t pt_pixel_seed(uint64_t base_seed, int32_t x, int32_t y);
/* RandomEngine(seed) raw state (base.h:26). */
uint64_t pt_rng_seed_to_state(uint64_t seed);

/* toneMap / gammaCorrect / postProcess (include/PathTrace/post_processing.h:14,22,30; src/post_processing.cpp:32-187) on an
 * rgba f32 frame (row-major, y * width + x as image/image.h:82), in place.  `steps` = PT_POST_TONE_MAP | PT_POST_GAMMA; both =
 * postProcess (tone mapping first).  `gamma` is gammaCorrect's argument (the reference's default is 1.8).
 * pt_post_process takes a HOST buffer (uploads, processes, downloads); pt_post_process_device works on DEVICE memory and is
 * ordered on `stream` (a hipStream_t, NULL = the default stream), which it synchronises before returning. */
#define PT_POST_TONE_MAP 1u
#define PT_POST_GAMMA 2u
int pt_post_process(int device, float *rgba, int32_t width, int32_t height, uint32_t steps, float gamma);
int pt_post_process_device(int device, float *d_rgba, int32_t width, int32_t height, uint32_t steps, float gamma, void *stream);

/* Feature-guided denoising of a finished frame (what RenderOptions::allow_bias asks for).
 *
 * pt_render_features: first-hit features of every pixel of the frame `options` describes (only image_width and image_height are read).
 * Each pixel traces 4 deterministic primary rays, at sub-pixel offsets (-1/4, -1/4), (+1/4, -1/4), (-1/4, +1/4), (+1/4, +1/4), through
 * `camera` with its aperture sampler ignored; the rays are a pure function of camera and pixel.  out_features: [height][width][3][4] floats,
 * each the mean over the 4 rays (a miss adds zeros):
 *   [0] = albedo rgb (diffuse for Lambertian, specular for glass and mirror, white for PT_NO_MATERIAL), fraction of the rays that hit
 *   [1] = shading normal xyz, hit distance t
 *   [2] = hit position xyz, luminance (0.2126 r + 0.7152 g + 0.0722 b) of the material's emission
 * Serialised on the scene like every render call.  The _device form writes into DEVICE memory, ordered on `stream` (a hipStream_t, NULL = the
 * library's own stream followed by a synchronisation) as pt_render_tiles_device.
 *
 * pt_denoise: an edge-avoiding a-trous filter guided by those features -- the spatial part of SVGF (Schied et al. 2017): demodulate by the
 * albedo, a per-pixel luminance variance from an edge-aware 3x3 neighbourhood, `iterations` passes of the 5x5 B3-spline kernel at step 2^i
 * with normal, depth and luminance weights, remodulate.  rgba and out_rgba: [height][width][4] floats; out_rgba may equal rgba; alpha is
 * copied unchanged.  fp32, deterministic, no atomics.  params NULL = pt_denoise_params_default; a sigma of 0 turns its term off.  The
 * _device form works on DEVICE memory, ordered on `stream` (NULL = the default stream), which it synchronises before returning.  The
 * scratch buffers belong to the library (one set per device, grown on demand, one call at a time per device).
 * PT_ERR_INVALID before anything is uploaded or launched: a null pointer, a size <= 0, more than 0x0fffffff pixels, iterations outside
 * 0..10, a negative or non-finite sigma. */
typedef struct pt_denoise_params {
    int32_t iterations;    /* a-trous passes, 0..10 */
    float sigma_luminance; /* luminance edge-stopping, in standard deviations of the local luminance */
    float sigma_normal;    /* exponent of max(0, n_p . n_q) */
    float sigma_depth;     /* depth edge-stopping, in units of the depth change the local gradient predicts */
} pt_denoise_params;
/* 5 passes, sigma_luminance 32, sigma_normal 128, sigma_depth 1: SVGF's defaults but for sigma_luminance (4 there), which is wider here
 * because the variance comes from one low-sample frame, not from temporal moments */
int pt_denoise_params_default(pt_denoise_params *out);
int pt_render_features(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, float *out_features);
int pt_render_features_device(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, float *d_out_features, void *stream);
int pt_denoise(int device, const float *rgba, const float *features, int32_t width, int32_t height, const pt_denoise_params *params, float *out_rgba);
int pt_denoise_device(int device, const float *d_rgba, const float *d_features, int32_t width, int32_t height, const pt_denoise_params *params,
                      float *d_out_rgba, void *stream);

/* The same for a batch of n_views frames of one size (a view batch: pt_render_views, pt_frame_create_views), ONE launch per stage for all
 * views: 1 feature launch, 3 + iterations filter launches, whatever n_views is.  features: [n_views][height][width][3][4]; rgba and out_rgba:
 * [n_views][height][width][4].  View v of each result is bit for bit what pt_render_features(cameras[v]) or pt_denoise on view v alone gives:
 * a neighbour or tap counts only if it lies in the same view, everything else is the same arithmetic in the same order.  n_views == 1 is the
 * single-frame entry point.  PT_ERR_INVALID as for those, and for n_views <= 0 or more than 0x0fffffff pixels over all views. */
int pt_render_features_views(pt_scene *scene, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, float *out_features);
int pt_render_features_views_device(pt_scene *scene, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, float *d_out_features,
                                    void *stream);
int pt_denoise_views(int device, const float *rgba, const float *features, int32_t width, int32_t height, int32_t n_views,
                     const pt_denoise_params *params, float *out_rgba);
int pt_denoise_views_device(int device, const float *d_rgba, const float *d_features, int32_t width, int32_t height, int32_t n_views,
                            const pt_denoise_params *params, float *d_out_rgba, void *stream);

/* The frame as it stands: what a viewer shows between two pt_frame_render calls.  `image` is the buffer the caller passes
 * to pt_frame_render (it holds the finished pixels); out_rgba is [height][width][4] floats and may equal `image` only when the caller no
 * longer needs the frame's own image (the next pt_frame_render would keep the preview's values in its unfinished pixels).  out_samples
 * is [height][width] int32 or NULL.  Per pixel:
 *   - finished: rgba copied from `image` bit for bit; samples = -1.
 *   - parked: the plain running mean of its estimator, pixel_value * (1 / collected_sample_count) in fp32 (the first step of the finish:
 *     alpha is 1), or (0, 0, 0, 0) if no sample was collected; samples = the samples the pixel has taken (>= 1).  A pixel whose
 *     estimator holds closed candidates may finish at another value: the preview never applies the candidate rule.
 *   - untouched, or in no tile of the frame: a hole, (0, 0, 0, 0); samples = 0.  Before the first pt_frame_render every pixel is a hole.
 * A complete frame previews as `image` bit for bit, every sample count -1.  Every replica gathers its parked pixels on its own device.
 * denoise != NULL: the preview is then filtered as pt_denoise filters a frame, with those parameters, on replica 0's device and with the
 * frame's first-hit features (pt_render_features with the frame's camera and size: computed on the first denoised preview and kept on
 * the device until pt_frame_destroy).  Holes are never taps of another pixel; a hole takes the normalised weighted mean of its other taps
 * in every pass (its own weight 0, no luminance term) and then has alpha 1, or stays (0, 0, 0, 0) if no pass found one.  Without holes
 * the result equals pt_denoise of the raw preview bit for bit.  out_samples is the raw preview's either way.
 * The preview changes nothing the frame will do, and takes the frame's lock (scene work is serialised with the scene's other calls).
 * PT_ERR_INVALID before any device is touched: null frame, image or out_rgba, or denoise parameters pt_denoise refuses; a failed
 * frame returns its stored status. */
int pt_frame_preview(pt_frame *frame, const float *image, const pt_denoise_params *denoise, float *out_rgba, int32_t *out_samples);
/* The measured variance of a frame's unfinished pixels (pt_frame_get_variance) and the filter fed with it (pt_denoise_measured,
 * pt_frame_preview_measured): struct pt_denoise_measured_params and those entry points are declared, with their contracts, in: */
#include "pt_frame_variance.h"
/* Denoiser features that follow mirrors and glass to the first diffuse hit (pt_render_features_followed*, pt_frame_set_feature_params;
 * DESIGN.md 4.10.2): struct pt_feature_params and those entry points are declared, with their contracts, in: */
#include "pt_features.h"
/* Checkpoints of a frame: save it into a blob, load the blob onto any number of replicas, finish bit-identically (pt_checkpoint_inspect,
 * pt_frame_checkpoint_size / _save / _load): the format, the structs and the entry points are declared in: */
#include "pt_checkpoint.h"
/* Scenes from indexed meshes instantiated under transforms, assembled on the device (pt_scene_create_meshes, pt_mesh_assemble,
 * pt_scene_instance_ranges, pt_scene_get_triangles): the structs and entry points are declared, with their contracts, in: */
#include "pt_mesh.h"
/* Re-posing the instances of such a scene in place, and the batched assembler behind it (pt_scene_pose, pt_scene_get_pose,
 * pt_mesh_assemble_batch): the struct and entry points are declared, with their contracts, in: */
#include "pt_pose.h"
/* Deforming the meshes of such a scene in place -- new vertices from the caller, or a bound rig skinned on the device -- followed by what
 * a pose does: the structs and entry points are declared, with their contracts, in: */
#include "pt_deform.h"
/* Blend shapes for the meshes of such a scene -- a bound set of morph targets weighted on the device, alone or in front of the bound rig
 * in one launch -- followed by what a pose does: the structs and entry points are declared, with their contracts, in: */
#include "pt_morph.h"
/* Where the surface a pixel sees was at the previous pose, and the temporal push that reprojects that point (pt_motion_table,
 * pt_render_features_motion, pt_temporal_denoise_motion): the entry points are declared, with their contracts, in: */
#include "pt_motion.h"
/* The same for meshes that were deformed or morphed between two frames: the scene keeps a mark of the previous frame and the feature
 * pass reprojects per vertex (pt_scene_motion_mark, pt_render_features_motion_marked): the entry points are declared,
 * with their contracts, in: */
#include "pt_motion_shapes.h"
/* A new look for such a scene in place -- materials, point lights, the material of an instance -- with the tree untouched and the emitter
 * registry rebuilt on the device (pt_scene_relight, pt_scene_get_materials, pt_scene_get_point_lights): the structs and
 * entry points are declared, with their contracts, in: */
#include "pt_relight.h"

/* Temporal denoising of a sequence of frames of one scene (a camera path, a turntable): the temporal half of SVGF (Schied et al. 2017)
 * in front of pt_denoise's spatial filter.  The entry points below reproject as for a scene that does not move; for a
 * scene posed between the frames (pt_scene_pose) the motion forms of include/pt_motion.h reproject through the poses.
 * A pt_temporal handle keeps the history of the frames pushed so far, on its own
 * device buffers (two handles may be interleaved).  Each push of a frame, its pt_render_features and its camera:
 *   - reprojects every covered pixel's mean hit position into the previous push's camera (a pinhole: the feature rays ignore the aperture)
 *     and takes the 2x2 bilinear taps there.  A tap is kept if it lies in the image, has the pixel's class (covered, emissive), a normal with
 *     dot >= normal_min and a position within position_tolerance pixel footprints (hit distance * height / (focal_length * image height)).
 *     A camera equal to the previous one bit for bit makes each pixel its own tap.
 *   - blends the demodulated colour and the luminance moments with the kept taps' history, weights renormalised:
 *     (1 - a) h + a x, a = max(1/n, alpha), n = min(1 + the taps' longest history, max_history); n = 1 (no valid tap) keeps x.
 *   - filters as pt_denoise with params.spatial, but where n >= max(2, moments_min_history) the luminance variance is mu2 - mu1^2 of the
 *     moments and the luminance sigma is sigma_luminance_temporal.  The output of the first a-trous pass is the next push's colour history.
 * A push without history (the first, the first after pt_temporal_reset, or one whose every tap was rejected) equals pt_denoise(params.spatial)
 * bit for bit.  rgba, features, out_rgba as for pt_denoise (out_rgba may equal rgba); out_history (may be NULL): [height][width] int32 n,
 * 0 where no ray hit.  fp32, deterministic, no atomics.  The _device form takes DEVICE memory and is ordered on `stream` (NULL = the default
 * stream), which it synchronises before returning.  Calls on one handle are serialised.
 * PT_ERR_INVALID before anything touches a device: a null pointer, a size <= 0 or above 0x0fffffff pixels, an alpha outside (0, 1],
 * max_history or moments_min_history < 1, spatial parameters pt_denoise refuses, a negative or non-finite sigma_luminance_temporal or
 * position_tolerance, a non-finite normal_min, or a camera whose basis is degenerate (non-finite, or forward, up and right not independent). */
typedef struct pt_temporal_params {
    pt_denoise_params spatial;      /* the spatial filter of every push */
    float alpha_color;              /* lower bound of the colour's blend weight, (0, 1] */
    float alpha_moments;            /* ... of the luminance moments', (0, 1] */
    int32_t max_history;            /* history length cap, >= 1 */
    int32_t moments_min_history;    /* history length from which the variance is temporal, >= 1 */
    float sigma_luminance_temporal; /* luminance sigma at those pixels */
    float normal_min;               /* least dot product of the normals of a kept tap */
    float position_tolerance;       /* largest distance of a kept tap's position, in pixel footprints */
} pt_temporal_params;
/* spatial = pt_denoise_params_default, alpha_color = alpha_moments = 0.2, max_history 32, moments_min_history 4 (SVGF's), and
 * sigma_luminance_temporal 4, normal_min 0.9, position_tolerance 2 */
int pt_temporal_params_default(pt_temporal_params *out);
typedef struct pt_temporal pt_temporal;
/* params NULL = pt_temporal_params_default */
int pt_temporal_create(int device, int32_t width, int32_t height, const pt_temporal_params *params, pt_temporal **out);
int pt_temporal_denoise(pt_temporal *t, const float *rgba, const float *features, const pt_camera_params *camera, float *out_rgba, int32_t *out_history);
int pt_temporal_denoise_device(pt_temporal *t, const float *d_rgba, const float *d_features, const pt_camera_params *camera, float *d_out_rgba,
                               int32_t *d_out_history, void *stream);
/* forgets the history: the next push has none */
int pt_temporal_reset(pt_temporal *t);
int pt_temporal_destroy(pt_temporal *t);

/* Light gathered at surface points -- ambient occlusion, direct light, full paths -- for points, for a frame's first hits and for the
 * corners of a mesh instance's triangles (pt_gather_points, pt_gather_frame, pt_gather_instance): declared, with their
 * contracts, in: */
#include "pt_gather.h"

/* Radiance along rays the caller chooses, and captures -- images of such rays made on the device by an equirectangular, cube-map, fisheye
 * or orthographic camera model (pt_radiance_rays, pt_radiance_capture): declared, with their contracts, in the file below.
 * Its last line includes pt_light_passes.h: the same samples split into passes by emitter group and bounce depth, and the mix of such
 * passes (pt_light_passes_rays, pt_light_passes_capture, pt_light_passes_mix). */
#include "pt_radiance.h"

/* Light probes -- the radiance that arrives at free points projected onto spherical harmonics, grids of such probes and the lookup that
 * shades a point with a normal from a grid (pt_light_probes_points, pt_light_probes_grid, pt_light_probes_shade):
 * declared, with their contracts, in: */
#include "pt_light_probes.h"

/* Scene queries: the hit record of a ray, of a pixel or of every pixel of a frame -- object, instance, face, position, normals,
 * barycentrics -- and occlusion tests of segments (pt_query_rays, pt_query_pixels, pt_query_frame, pt_occluded_rays): the
 * record and the entry points are declared, with their contracts, in the file below.  Its last line includes pt_nearest.h: the question
 * that follows no ray -- the closest point of the scene's surfaces to a free point, with distance, object, instance, face, barycentrics
 * and the feature it lies on, and unsigned distance grids (pt_nearest_points, pt_distance_grid_fill). */
#include "pt_query.h"

#ifdef __cplusplus
}
#endif

#endif /* PT_HIP_H */
