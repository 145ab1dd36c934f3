// pt_host.h -- what the host units of libpathtrace_hip.so share: pt_api.cpp (scenes), pt_meshes.cpp (scenes from meshes and instances),
// pt_pose.cpp (their instances under new matrices, in place), pt_deform.cpp (their meshes under new vertices, in place),
// pt_morph.cpp (their meshes under blend shapes, in place),
// pt_relight.cpp (their materials and lights replaced in place), pt_motion.cpp and pt_motion_shapes.cpp (motion for the temporal denoiser),
// pt_query.cpp (hit records and occlusion tests), pt_nearest.cpp (the nearest surface to free points, distance grids), pt_gather.cpp (light gathered at points; with pt_light_probes.cpp, pt_radiance.cpp and
// pt_light_passes.cpp it takes its launch frame from pt_sample_host.h, which sits on top of this header),
// pt_render.cpp (render calls), pt_frames.cpp and pt_frame_maps.cpp (resumable frames and their maps; pt_frames.h) and pt_image.cpp
// (post-processing, features, denoising).  Internal:
// not installed, not part of the C ABI.  Everything but the ABI's own handle types lives in namespace pth, so that no helper can collide
// with a pt_* name of include/pt_hip.h.
#ifndef PT_HOST_H
#define PT_HOST_H

#include "../../include/pt_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pt_build.h"
#include "pt_mesh.h"
#include "pt_mesh_batch.h"
#include "pt_skin.h"
#include "pt_morph_skin.h"
#include "pt_bvh.h"
#include "pt_kernels.h"
#include "pt_denoise.h"
#include "pt_post.h"

namespace pth {

// The calling thread's message (pt_last_error).  It has one definition, in pt_api.cpp, and is reached through these two only: a copy
// per unit would hand pt_last_error() another unit's empty string.
int fail(int code, const std::string &msg);
const std::string &last_error();

#define PT_HIP(call)                                                                                               \
    do {                                                                                                           \
        hipError_t err_ = (call);                                                                                  \
        if(err_ != hipSuccess) {                                                                                   \
            return fail(PT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(err_));                          \
        }                                                                                                          \
    } while(0)

// ... and for a helper that returns a status of its own (it has set the message)
#define PT_TRY(call)                                                                                               \
    do {                                                                                                           \
        const int rc_ = (call);                                                                                    \
        if(rc_ != PT_OK) {                                                                                         \
            return rc_;                                                                                            \
        }                                                                                                          \
    } while(0)

// ... and for a launch wrapper of a kernel file that returns 0, or 1 when a launch failed
#define PT_LAUNCH(call, what)                                                                                      \
    do {                                                                                                           \
        if((call) != 0) {                                                                                          \
            PT_HIP(hipGetLastError());                                                                             \
            return fail(PT_ERR_HIP, what);                                                                         \
        }                                                                                                          \
    } while(0)

inline int env_int(const char *name, int fallback) {
    const char *v = std::getenv(name);
    return (v != nullptr && *v != '\0') ? std::atoi(v) : fallback;
}

inline float fmin_std(float a, float b) {
    return (b < a) ? b : a;
}
inline float fmax_std(float a, float b) {
    return (a < b) ? b : a;
}

struct Vec3 {
    float x, y, z;
};
inline Vec3 sub(Vec3 a, Vec3 b) {
    return {a.x - b.x, a.y - b.y, a.z - b.z};
}
inline Vec3 scale(Vec3 a, float f) {
    return {a.x * f, a.y * f, a.z * f};
}
inline float dot(Vec3 a, Vec3 b) {
    float d = 0.0F;
    d += a.x * b.x;
    d += a.y * b.y;
    d += a.z * b.z;
    return d;
}
inline Vec3 cross(Vec3 a, Vec3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
inline Vec3 normalize(Vec3 a) {
    const float inv = 1.0F / std::sqrt(dot(a, a));
    return scale(a, inv);
}
inline Vec3 ld(const float *p) {
    return {p[0], p[1], p[2]};
}

inline uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
inline float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

template<typename T>
struct DevBuf {
    T *ptr = nullptr;
    size_t count = 0;
    ~DevBuf() { release(); }
    void release() {
        if(ptr != nullptr) {
            (void)hipFree(ptr);
            ptr = nullptr;
            count = 0;
        }
    }
    hipError_t ensure(size_t n) {
        if(n <= count && ptr != nullptr) {
            return hipSuccess;
        }
        release();
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&ptr), bytes);
        if(e == hipSuccess) {
            count = std::max<size_t>(n, 1);
        }
        return e;
    }
    hipError_t upload(const std::vector<T> &host) {
        hipError_t e = ensure(host.size());
        if(e != hipSuccess || host.empty()) {
            return e;
        }
        return hipMemcpy(ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

// to takes from's memory over (what it had is freed)
template<typename T>
void take(DevBuf<T> &to, DevBuf<T> &from) {
    to.release();
    to.ptr = from.ptr;
    to.count = from.count;
    from.ptr = nullptr;
    from.count = 0;
}

struct F4 {
    float x, y, z, w;
};

// A stream of a call's own, destroyed with the call
struct StreamGuard {
    hipStream_t stream = nullptr;
    ~StreamGuard() {
        if(stream != nullptr) {
            (void)hipStreamDestroy(stream);
        }
    }
};

struct Event {
    hipEvent_t e = nullptr;
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
    ~Event() {
        if(e != nullptr) {
            (void)hipEventDestroy(e);
        }
    }
};

// The device time of what a stream does between begin() and end(): ms(), once the stream has been synchronised
struct EventPair {
    Event first, last;
    hipError_t begin(hipStream_t stream) {
        hipError_t err = first.create();
        if(err == hipSuccess) {
            err = last.create();
        }
        return err == hipSuccess ? hipEventRecord(first.e, stream) : err;
    }
    hipError_t end(hipStream_t stream) { return hipEventRecord(last.e, stream); }
    hipError_t ms(float *out) { return hipEventElapsedTime(out, first.e, last.e); }
};

// ---- what a scene with mesh instances keeps for pt_scene_pose (pt_pose.cpp; include/pt_pose.h has the memory cost) --------------------------

// What pt_scene_deform (pt_deform.cpp; include/pt_deform.h has the memory cost) adds to a mesh: the rig bound to it, and its current
// vertices with the spare buffer the next deformation is made in.  A mesh that was never bound or deformed has none.
struct MeshDeform {
    DevBuf<uint32_t> skin_bone; // [n_vertices][skin_k]
    DevBuf<float> skin_weight;  // [n_vertices][skin_k]
    uint32_t skin_bones = 0, skin_k = 0; // skin_bones == 0: no skin
    DevBuf<float> current, spare;        // [n_vertices][3] each
    // ... and what pt_scene_bind_morphs (pt_morph.cpp; include/pt_morph.h) binds: the set's entries vertex-major
    DevBuf<uint32_t> morph_row_start;    // [n_vertices + 1]
    DevBuf<PtMorphEntry> morph_entries;  // [morph_entry_count], a vertex's in ascending target order
    uint32_t morph_targets = 0;          // 0: no set
    uint64_t morph_entry_count = 0;
    // ... and what pt_scene_motion_mark (pt_motion_shapes.cpp; include/pt_motion_shapes.h) keeps of a deformed mesh: the current vertices
    // it had at the mark, allocated by the mesh's first such mark and reused
    DevBuf<float> marked;                // [n_vertices][3]
};

// One mesh in device memory
struct KeptMesh {
    DevBuf<float> vertices; // the rest vertices
    DevBuf<int32_t> faces;
    uint32_t n_vertices = 0, n_faces = 0;
    // The vertices an assembly reads (assemble_batch, pt_meshes.cpp): the rest vertices, unless pt_scene_deform has pointed it at the
    // mesh's current ones
    const float *shape = nullptr;
    uint64_t shape_serial = 0; // bumped by adopt_shapes (pt_deform.cpp) for every mesh whose shape a successful call changed
    std::unique_ptr<MeshDeform> deform;
    int upload(const pt_mesh_data &m);
};

// A deep copy of a scene description: create_scene reads the description's host arrays (emitters, materials, the host builder's boxes)
struct DescCopy {
    pt_scene_desc d{};
    std::vector<uint8_t> obj_kind, tri_cull;
    std::vector<float> tri_pos, tri_nrm, sph, light_pos, light_spectrum;
    std::vector<uint32_t> tri_material, sph_material;
    std::vector<pt_material> materials;
    void assign(const pt_scene_desc &src);
};

// What pt_scene_motion_mark (pt_motion_shapes.cpp) records, "the previous frame", and what the scene tracks while there is one: the
// scene-wide face every instance triangle came from.  A scene that was never marked has none of this.
struct MotionMark {
    std::vector<float> transforms;      // [n_instances][16]: the instance matrices at the mark
    std::vector<const float *> shape;   // per mesh: its vertices at the mark -- the rest array, or the mesh's `marked` buffer; null: unused mesh
    std::vector<uint64_t> serial;       // per mesh: its shape_serial at the mark
    // face_of[t] for instance triangle t, written by every successful rebuild since the first mark (has_table); a rebuild makes the
    // table in `face_of_spare` and they change places at adoption
    DevBuf<uint32_t> face_of, face_of_spare;
    bool has_table = false;
    DevBuf<PtShapeMotionInstance> table; // the instance table of the last marked features call
};

struct PoseKeep {
    std::vector<std::unique_ptr<KeptMesh>> meshes; // by mesh index of the creating call; null for a mesh no instance uses
    std::vector<pt_mesh_instance> instances;
    DescCopy desc;
    bool any_smooth = false;
    uint64_t capacity = 0;               // the description's triangles + the faces of all instances, before any is rejected
    PtBatchScratch scratch;              // the assembler's, grown by the first pose (creation has one of its own, freed when it returns)
    DevBuf<float> spare_pos, spare_nrm;  // the arrays the next pose assembles into (the scene keeps the positions it was built from)
    DevBuf<float> bone_table;            // pt_scene_deform: the bone matrices of a call's skinned meshes, end to end
    DevBuf<float> morph_weights;         // pt_scene_morph: the weights of a call's morphed meshes, end to end
    uint64_t deform_allocations = 0;     // ... and its hipMalloc calls for vertex, skin and bone buffers so far
    std::unique_ptr<MotionMark> mark;    // pt_scene_motion_mark: null for a scene that is not marked
};

} // namespace pth

struct pt_scene {
    int device = 0;
    hipStream_t stream = nullptr;
    int cu_count = 256;

    // host copies kept for introspection and for mapping references back to object indices
    ptb::Tree tree;          // host-built scenes only (PT_BUILD=host or few objects); empty when the device built the tree
    uint64_t n_nodes = 0;    // 2 * n_objects - 1
    uint32_t depth = 0;      // levels of the tree (a single leaf has depth 1)
    bool device_built = false;
    float build_ms[4] = {0, 0, 0, 0}; // host preparation, upload, device tree construction, emissive registration + rest
    std::vector<uint32_t> tri_obj; // object of every triangle of the description; the triangles of mesh instances follow them and need no table:
    std::vector<uint32_t> sph_obj;
    uint32_t n_objects = 0;
    uint32_t n_desc_objects = 0, n_desc_tris = 0; // ... triangle n_desc_tris + k is object n_desc_objects + k (pt_scene_create_meshes)
    uint32_t tri_object(uint32_t t) const { return t < tri_obj.size() ? tri_obj[t] : n_desc_objects + (t - n_desc_tris); }
    // scenes of pt_scene_create_meshes with instances: their object ranges, the triangle or sphere of every object of the description
    // (PT_REF_SPHERE | index), and the triangles' positions as the builder took them (pt_scene_get_triangles)
    std::vector<uint32_t> inst_first, inst_count, desc_ref;
    pth::DevBuf<float> tri_pos_kept;
    // ... and for pt_scene_relight (pt_relight.cpp) the depth-first order of the leaves in device memory -- the device builder's array,
    // or the host tree's order uploaded by the first relight -- and, from the first relight on, desc_ref
    pth::DevBuf<uint32_t> leaf_order, desc_ref_dev;
    std::unique_ptr<pth::PoseKeep> pose;      // ... and their meshes, instance table and description, for pt_scene_pose
    std::atomic<uint32_t> live_frames{0};     // pt_frame handles (replicas counted) on this scene: pt_scene_pose refuses while there is one
    uint32_t n_emissive = 0;
    std::vector<int32_t> emissive_obj;
    std::vector<float> emissive_cdf;

    // device scene
    pth::DevBuf<pth::F4> recs, pairs, tris, tri_shade, spheres, materials, lights, emis; // (pairs and tris only while the scene is being built: linked into recs)
    pth::DevBuf<uint2> sph_meta;
    pth::DevBuf<float> emis_cdf;
    PtDevScene dev{};

    pth::DevBuf<PtDevCounters> counters;
    pth::DevBuf<pth::F4> image;
    pth::DevBuf<int4> tiles;
    pth::DevBuf<uint32_t> tile_offset;
    pth::DevBuf<float> batch_rays;

    // One render call at a time per scene: the workspace below is shared by every entry point (processItem may be called from several
    // threads on one const Scene, reference worker.h:66-69 / src/worker.cpp:328-362: such callers are serialised here).
    std::mutex render_mutex;

    // workspace of the persistent path kernel (pt_path.hip), grown on demand and reused between calls
    PtPathConfig path_cfg{};
    int path_blocks_per_cu = 0;
    uint32_t path_slots = 0, path_waves = 0, path_cap = 0;
    pth::DevBuf<uint32_t> sl_nee_mask, pull_counter, tile_left;
    pth::DevBuf<int4> st_rect;
    pth::DevBuf<uint64_t> st_rng;
    pth::DevBuf<pth::F4> sl_state, sl_nee, lq_ray_o, lq_ray_d;
    pth::DevBuf<PtEstimator> sl_est;
    pth::DevBuf<PtCandidate> sl_cand;
    pth::DevBuf<uint2> path_spill, closest_out;
    pth::DevBuf<uint32_t> walk_save;
    pth::DevBuf<PtPathArgs> path_args;  // the kernel's arguments in device memory
    PtPathArgs host_path_args{};   // ... and the host copy they are uploaded from
    pth::DevBuf<unsigned long long> path_wave_counters;
    uint32_t *host_tiles_done = nullptr; // pinned: tiles finished so far, written by the kernel (progress callback)
    unsigned long long *host_streams_done = nullptr; // pinned: the launch's count of finished streams, copied behind every launch
    uint64_t streams_expected = 0;                   // ... and what it must read once the stream has drained (finish_path)
    // a controlled launch (pt_render_tiles_ctl) also leaves its count of abandoned streams in host_streams_done[1] and its final pull
    // counter in host_streams_done[2]; finish_path accounts for every stream with them
    bool streams_controlled = false;
    uint32_t streams_first_total = 0;
    uint32_t *host_cancel = nullptr; // pinned, fine-grained: the stop request of a controlled launch (PtStreams::cancel), written by the host
    uint32_t *dev_cancel = nullptr;  // ... and its address on the device
    // cost-aware placement (render_tiles_impl): what every stream of the pilot launch cost, and the stream every slot of the main launch starts with
    pth::DevBuf<uint32_t> sl_cost, stream_cost, place;
    // a view batch (pt_render_views): the cameras and seeds of its views
    pth::DevBuf<PtViewCamera> view_cams;
    pth::DevBuf<uint64_t> view_seeds;
    // the first-hit features of a frame (pt_render_features*): the frame's features and the walks' spill area
    pth::DevBuf<pth::F4> features;
    pth::DevBuf<uint2> feature_spill;
    pth::DevBuf<PtViewCamera> feature_cams; // pt_render_features_views: the views' cameras, aperture none
    // pt_render_features_motion (pt_motion.cpp): the host form's motion plane and the instance table of the call
    pth::DevBuf<pth::F4> motion;
    pth::DevBuf<PtMotionInstance> motion_instances;
    // scene queries (pt_query.cpp; include/pt_query.h): the host forms' queries, records and flags, the walks' spill area, and the
    // instance table with the object ranges it was made from (it is made again when the scene's ranges differ from them)
    pth::DevBuf<float> query_in;
    pth::DevBuf<pt_hit> query_out;
    pth::DevBuf<uint8_t> query_flags;
    pth::DevBuf<uint2> query_spill;
    pth::DevBuf<PtQueryInstance> query_instances;
    std::vector<uint32_t> query_inst_first, query_inst_count;
    uint32_t query_n_instances = 0;
    bool query_table_made = false;
    // nearest-surface queries (pt_nearest.cpp; include/pt_nearest.h): the host forms' points, records and grid planes; the walks spill
    // into query_spill, ordered by the scene's stream like the queries above
    pth::DevBuf<float> nearest_in, nearest_distance;
    pth::DevBuf<pt_nearest> nearest_out;
    pth::DevBuf<int32_t> nearest_object;
    // light gathered at points (pt_gather.cpp; include/pt_gather.h): the host forms' points and records, the points and the missing
    // pixels of a frame or an instance, and the workspace of one launch: the samples' plane or bits and the walks' spill area
    pth::DevBuf<float> gather_points;
    pth::DevBuf<uint8_t> gather_miss;
    pth::DevBuf<pt_gather_result> gather_out;
    pth::DevBuf<pth::F4> gather_plane;
    pth::DevBuf<unsigned long long> gather_bits;
    pth::DevBuf<uint2> gather_spill;
    bool debug_collect_costs = false;                // pt_debug_collect_costs: every launch records them
    std::vector<uint32_t> debug_place;               // pt_debug_set_place: the next launch starts from this table ...
    uint32_t debug_place_waves = 0, debug_place_slots = 0; // ... with this many wavefronts and slots in each

    ~pt_scene() {
        if(host_tiles_done != nullptr) {
            (void)hipHostFree(host_tiles_done);
        }
        if(host_streams_done != nullptr) {
            (void)hipHostFree(host_streams_done);
        }
        if(host_cancel != nullptr) {
            (void)hipHostFree(host_cancel);
        }
        if(stream != nullptr) {
            (void)hipStreamDestroy(stream);
        }
    }
};

namespace pth {

// ---- pt_api.cpp ------------------------------------------------------------------------------------------------------------------------

int device_count_quiet();
int check_device(int device); // PT_ERR_NO_DEVICE without a HIP device, or for an index that names none
PtDevCamera derive_camera(const pt_camera_params *c);
int derive_options(const pt_options *o, PtDevOptions *out);
int check_render_args(pt_scene *scene, const pt_camera_params *camera, const pt_options *options);

// Triangles that are in device memory already (assemble_mesh_scene, pt_meshes.cpp): those of the description first, then the ranges of the
// mesh instances, each with one cull flag and one material.
struct DeviceTriangles {
    const float *pos = nullptr; // [n_triangles][9]
    const float *nrm = nullptr; // [n_triangles][9] or null: face normals
    uint32_t n_triangles = 0;   // the description's and the ranges'
    std::vector<PtBatchRange> ranges; // one per instance, in order (sorted by first_tri, empty ones included)
    hipEvent_t ready = nullptr;       // the arrays are complete once this event of the assembly's stream is
    // The ranges' constants are filled in one launch on the new scene's stream, which reads the range table from this scratch: it stays
    // alive, and is not used again, until that stream has been waited for
    PtBatchScratch *scratch = nullptr;
};
// Whether a scene of n_objects is built on the device (PT_BUILD_DEVICE_MIN, PT_BUILD)
bool builds_on_device(uint32_t n_objects);
// pt_scene_create; with `assembled` (device builder only) the triangles are taken from device memory: d's own per-triangle arrays tri_pos
// and tri_nrm are not read, and nothing per triangle of the ranges crosses to the host but the positions of the emissive ones.
int create_scene(int device, const pt_scene_desc *d, const DeviceTriangles *assembled, pt_scene **out);
// What create_scene derives from a look, for pt_scene_relight to derive again: the material and the light table as the device reads them
// (4 and 2 float4 each), the emitter samples per path vertex of a registry of n_emissive objects (scene.cpp:226), and whether the scene
// is staged in LDS (dev.n_lds_pairs / n_lds_tris, from the record counts, n_lights and n_object_samples of dev)
std::vector<F4> material_table(const pt_material *materials, uint32_t n);
std::vector<F4> light_table(const float *pos, const float *spectrum, uint32_t n);
int object_samples(uint32_t n_emissive);
void stage_small_scene(PtDevScene &dev);

// ---- pt_meshes.cpp ---------------------------------------------------------------------------------------------------------------------

int check_mesh(const pt_mesh_data *m);
// The front half of pt_scene_create_meshes and pt_scene_pose: the description's triangles at the front of pos / nrm (device memory, room
// for `capacity` triangles; nrm null: no normal array, the builder makes face normals), with face normals for them where the description
// has none, and behind them all instances through the batched assembler (pt_mesh_batch.h), chunk after chunk.  Everything is enqueued on
// `stream`, which is waited for once per chunk; the last chunk's corner sort and smoothing are still in flight when this returns:
// triangles.ready is their end.  `scratch` must outlive what finish_mesh_scene enqueues on the new scene's stream.
struct MeshAssembly {
    DeviceTriangles triangles;                    // what create_scene takes
    std::vector<uint32_t> inst_first, inst_count; // the instances' object ranges (pt_scene_instance_ranges)
    uint32_t chunks = 0;                          // one wait each
    EventPair chain;                              // the device time of the assembly, once `stream` has been waited for
    std::chrono::steady_clock::time_point front_done; // when the description's triangles had been handed over
};
// face_of (device memory, one word per face of all instances; null: not tracked): face_of[t] receives the scene-wide face -- the faces of
// all instances end to end, before rejection -- that became instance triangle t (pt_face_table_kernel behind every chunk).
int assemble_mesh_scene(hipStream_t stream, const pt_scene_desc *d, const std::vector<std::unique_ptr<KeptMesh>> &meshes, const std::vector<pt_mesh_instance> &instances,
                        PtBatchScratch &scratch, uint64_t capacity, float *pos, float *nrm, MeshAssembly *out, uint32_t *face_of = nullptr);
// From the assembled arrays to the finished scene, with either builder: `assembled` names the triangles in `pos` / `nrm` (device memory:
// the description's first, then the instances' ranges).  The scene takes `pos` over (pt_scene_get_triangles); on failure it stays
// with the caller.  Used by pt_scene_create_meshes and pt_scene_pose.
int finish_mesh_scene(int device, const pt_scene_desc *d, const MeshAssembly &assembly, DevBuf<float> &pos, pt_scene **out);

// ---- pt_pose.cpp -----------------------------------------------------------------------------------------------------------------------

// What pt_scene_pose and pt_scene_deform share once their arguments are in order (render_mutex held, no live frame, the scene's stream
// idle or holding only work the assembly may follow): all instances of s->pose under the matrices `posed` through the batched assembler,
// each mesh read at its `shape`; the scene of these triangles built aside; and, only when that is complete, its content moved into `s`,
// which keeps its address, stream, lock, pinned words and workspace buffers, with `posed` as its instance table.  A failure leaves `s`
// as it was.  The stream has been waited for when this returns.  `info` (may be null) receives what a pose reports; t_begin is the
// call's start, for its wall-clock fields.
int rebuild_instances(pt_scene *s, std::vector<pt_mesh_instance> &&posed, std::chrono::steady_clock::time_point t_begin, pt_pose_info *info);

// ---- pt_deform.cpp ---------------------------------------------------------------------------------------------------------------------

// What pt_scene_deform and pt_scene_morph (pt_morph.cpp) share.  The refusals of both, word for word:
extern const char *const DEFORM_NO_INSTANCES;
extern const char *const DEFORM_LIVE_FRAME;
// The mesh `mesh` of the creating call, if an instance uses it
int used_mesh(PoseKeep &keep, uint32_t mesh, KeptMesh **out);
// buf.ensure(n), counted in keep.deform_allocations when it allocates
template<typename T>
int ensure_counted(PoseKeep &keep, DevBuf<T> &buf, size_t n) {
    const bool allocates = !(n <= buf.count && buf.ptr != nullptr);
    PT_HIP(buf.ensure(n));
    if(allocates) {
        keep.deform_allocations++;
    }
    return PT_OK;
}
// The pose arguments of a deformation, checked as pt_scene_pose checks them (before any device work) ...
int check_pose_arguments(const PoseKeep &keep, const uint32_t *instances, uint32_t n);
// ... and the instance table they ask for
std::vector<pt_mesh_instance> posed_instances(const PoseKeep &keep, const uint32_t *instances, uint32_t n, const float *transforms);
// Both current and spare vertices of `mesh`, allocated by its first deformation and reused: they change places after every call
int ensure_vertex_buffers(PoseKeep &keep, KeptMesh &mesh);
// The back half of a deformation, once every named mesh has its new vertices in the buffer shape[m] names (null: mesh m is not named;
// in_spare[m]: the buffer is the mesh's spare one), made by work the scene's stream holds: the meshes' `shape` pointers are turned to
// them, rebuild_instances assembles all instances under `posed` behind that work without a host wait and adopts the finished scene,
// and only then do spare and current buffers change places; a failure turns the pointers back.  The stream has been waited for when
// this returns PT_OK.
int adopt_shapes(pt_scene *s, const std::vector<const float *> &shape, const std::vector<uint8_t> &in_spare, std::vector<pt_mesh_instance> &&posed,
                 std::chrono::steady_clock::time_point t_begin, pt_pose_info *info);
// Waits for `stream` when it goes out of scope armed: from its construction on the stream may hold work of a call that must not
// outlive the call
struct StreamDrain {
    hipStream_t stream;
    bool armed = true;
    ~StreamDrain() {
        if(armed) {
            (void)hipStreamSynchronize(stream);
        }
    }
};

// ---- pt_render.cpp: the persistent path kernel (pt_path.hip), one launch per render call ----------------------------------------------

// The stop of one controlled call (pt_render_tiles_ctl), shared by the host threads of its replicas.  The stop travels to the device as
// one word per replica in pinned, fine-grained host memory; the host loop of every launch polls the caller's cancel flag and the deadline,
// and the first one to see either writes 1 into the word of every replica whose launch is prepared or running.
struct RenderStop {
    typedef std::chrono::steady_clock Clock;
    pt_render_control none{}; // (a call without a control can still be asked to stop by its deadline -- it has none -- or not at all)
    pt_render_control *ctl;
    bool has_deadline = false;
    Clock::time_point deadline;
    std::atomic<bool> requested{false};
    std::mutex mutex; // guards what follows
    Clock::time_point requested_at;
    std::vector<uint32_t *> words; // the cancel words of the launches prepared or running
    double drain_ms = 0.0;         // the latest end of a launch after the request

    // The stop of a call that began at `start`: its deadline from ctl->budget_ms (ctl may be null), and a first look at both -- a control
    // cancelled before the call, or a budget spent already, starts the launches stopped.
    RenderStop(pt_render_control *ctl, Clock::time_point start);
    // a launch takes part: its word starts as the stop's state (a request that came before the launch stops it at its first pass)
    void enlist(uint32_t *word);
    // ... and has ended (seen by its host loop at `end`): its word may serve another call now
    void retire(uint32_t *word, Clock::time_point end);
    void poll();
};

// What a controlled launch did with its streams (finish_path)
struct StreamTally {
    uint64_t finished = 0, abandoned = 0, unclaimed = 0;
};

struct PathPlan;
int setup_path(pt_scene *s);
// Grid and slot rows for n streams, and the buffers they need.
int ensure_path_workspace(pt_scene *s, uint32_t n, PtPathConfig *out_cfg, const PathPlan *plan = nullptr);
// Render the streams described by T (device pointers) with one launch on the scene's stream.  With a progress function the host polls
// the count of finished tiles (pinned memory, written by the kernel) while the launch runs and reports every step from the calling thread.
// With a RenderStop (controlled launches) the host loop runs whether or not there is a progress function: it forwards a stop request to the
// launch through the scene's cancel word.
int run_path(pt_scene *s, const PtDevCamera &cam, const PtDevOptions &opt, PtStreams T, float4 *d_image, pt_stats *stats, pt_progress_fn progress, void *progress_user,
             RenderStop *stop = nullptr);
// Wait for the scene's stream and make sure the last launch rendered every stream it was given: a wavefront that left early or a stream
// lost in the hand-out would otherwise return stale pixels with PT_OK.  Every entry point that synchronises anyway ends with this.  A
// controlled launch must account for every stream as finished, abandoned or never taken; `tally` (may be null) receives the three.
int finish_path(pt_scene *s, StreamTally *tally = nullptr);

// A view batch (pt_render_views): n > 1 views of one scene whose frames are stacked into one image of n * image_height rows; view v has the
// camera cams[v] and the seed seeds[v].  The tiles of such a call lie in the stacked image.
struct ViewSet {
    std::vector<PtViewCamera> cams;
    std::vector<uint64_t> seeds;
    int32_t rows(const pt_options *options) const { return static_cast<int32_t>(cams.size()) * options->image_height; }
};

// The arguments every view-batch entry point checks before anything is launched; fills the stacked tile list and, for V > 1, the view set.
int prepare_views(const pt_camera_params *cameras, const uint64_t *base_seeds, int32_t n_views, const pt_options *options, std::vector<pt_tile> *tiles, ViewSet *views);

// Every tile lies inside the image of `rows` rows and is not empty; with `total`, the tiles' pixels are counted into it and may not be
// more than 0x0fffffff in one `unit` (the message's last word).
int check_tiles(const pt_tile *tiles, size_t n_tiles, int32_t width, int32_t rows, uint64_t *total, const char *unit = "call");

// The tile table of a launch, on the host: stream i = pixel i of the tiles laid end to end; the kernel derives rectangle and engine from it.
struct TileTable {
    std::vector<int4> rects;
    std::vector<uint32_t> offsets, left; // the first stream of every tile, and its pixels
    TileTable(const pt_tile *tiles, size_t n_tiles);
};
// The tile and view fields of a launch's streams, from the tables in device memory (the scene's for a render call, a frame's own for its
// launches); n_views <= 1: no view tables.
void set_tile_streams(PtStreams *T, uint32_t n, const int4 *d_tiles, const uint32_t *d_offset, size_t n_tiles, uint64_t base_seed, int32_t n_views, int32_t view_height,
                      const PtViewCamera *d_view_cams, const uint64_t *d_view_seeds);
// A regular grid of equal tiles (what pt_job_tiles makes of a frame whose sides are multiples of the tile size) lets the kernel spread a
// wavefront's first rows over the frame's columns as well as over its bands: tiles per grid row, 64-stream chunks per tile (0, 0: no grid).
void tile_grid(const pt_tile *tiles, size_t n_tiles, uint32_t *tiles_per_row, uint32_t *chunks_per_tile);
// The replica that renders each tile of a multi-device call (render_tiles_multi_impl, and a frame's tiles for good: pt_frame_create).
std::vector<int> tile_owners(const pt_tile *tiles, size_t n_tiles, int n_scenes);

// Runs fn(i) for the replicas i = 0 .. n-1 of a multi-device call, replica 0 on the calling thread and every other one on a thread of its
// own, and waits for all of them.  PT_OK, or the code of the first replica that failed with the message "scene i: " + its thread's message.
int for_each_replica(int n, const std::function<int(int)> &fn);

// The progress function of a multi-device call: its replicas' launches report through callback() / this, and the caller's function sees
// one count over all of them, one call at a time (from the replicas' polling threads).
struct SharedProgress {
    std::mutex mutex;
    int completed, total;
    pt_progress_fn fn;
    void *user;
    SharedProgress(pt_progress_fn fn_, void *user_, int completed_, int total_) : completed(completed_), total(total_), fn(fn_), user(user_) {}
    pt_progress_fn callback() const { return fn != nullptr ? &SharedProgress::step : nullptr; }
    static void step(int, int, void *shared);
};

// The rectangles of `tiles` between the caller's image (`width` pixels wide) and the scene's frame in HBM, on the scene's stream; with
// `skip`, tile k is left out when skip[index[k]] is set.
int copy_tile_rects(pt_scene *s, const std::vector<pt_tile> &tiles, const std::vector<size_t> &index, const uint8_t *skip, float *image, size_t width, bool to_device);

// The library's stream ordered after the caller's stream (begin), and the caller's later work after the library's (end: not called when
// the work between them failed to enqueue, so that the caller's stream is not made to wait then)
struct StreamOrder {
    Event ev;
    hipStream_t caller = nullptr, own = nullptr;
    int begin(void *caller_stream, hipStream_t own_stream) {
        caller = static_cast<hipStream_t>(caller_stream);
        own = own_stream;
        PT_HIP(ev.create(hipEventDisableTiming));
        PT_HIP(hipEventRecord(ev.e, caller));
        PT_HIP(hipStreamWaitEvent(own, ev.e, 0));
        return PT_OK;
    }
    int end() {
        PT_HIP(hipEventRecord(ev.e, own));
        PT_HIP(hipStreamWaitEvent(caller, ev.e, 0));
        return PT_OK;
    }
};

// ---- pt_motion.cpp ---------------------------------------------------------------------------------------------------------------------

// What pt_render_features_motion and the marked call of pt_motion_shapes.cpp share.  One instance of pt_motion_table: the kind, and for a
// moved instance back[12] and normal[9]; the identity (static) or zero (none) tables of the other kinds
uint8_t motion_of(const float *c, const float *p, float back[12], float normal[9]);
void motion_identity(uint8_t kind, float back[12], float normal[9]);
// The arguments of the features-with-motion entries, checked without a device
int motion_check(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const float *out_features, const float *out_motion);
// The device table of a call (render_mutex held) for the previous matrices `previous` (null: nothing moved); *n_out = 0: no table needed
int motion_instances(pt_scene *s, const float *previous, uint32_t *n_out);
// Enqueues pt_motion_kernel on the scene's stream (render_mutex held) with the table motion_instances left
int motion_launch(pt_scene *s, const pt_camera_params *camera, const pt_options *options, uint32_t n_instances, float4 *d_features, float4 *d_motion);

// ---- pt_query.cpp ----------------------------------------------------------------------------------------------------------------------

// The tables a record's instance and face are looked up in (render_mutex held, the device set), for pt_nearest.cpp as well: the
// instance table is made again only when the scene's ranges differ from the ones it was made from
int query_record_tables(pt_scene *s, PtQueryTables *out);

// ---- pt_radiance.cpp -------------------------------------------------------------------------------------------------------------------

// The refusals of include/pt_radiance.h, made without a device, for pt_light_passes.cpp as well: `out` is the array the call fills
// (needed where n > 0); *n_out = the capture's pixels
int radiance_check_params(const pt_radiance_params *p, uint64_t n);
int radiance_check_rays(pt_scene *s, const float *rays, size_t n, const pt_radiance_params *params, const void *out);
int radiance_check_capture(pt_scene *s, const pt_capture_desc *c, const pt_radiance_params *params, const void *out, uint64_t *n_out);
// A capture as the kernels take it (null: a 1 x 1 capture that no kernel reads)
PtCaptureParams radiance_device_capture(const pt_capture_desc *c);

// ---- pt_image.cpp ----------------------------------------------------------------------------------------------------------------------

// Enqueues the feature pass for the stacked frames of n_views cameras on the scene's stream (render_mutex held), in one launch: into
// `d_out`, n_views * width * height * 3 float4.  follow == nullptr: first-hit features (pt_feature_kernel); else the followed ones
// (pt_follow_kernel; include/pt_features.h) with parameters that feature_params_resolve has passed and options->epsilon.
int features_views_launch(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, float4 *d_out,
                          const pt_feature_params *follow = nullptr);
// The parameters of the followed feature entries (NULL = pt_feature_params_default) and the epsilon they read, checked without a device
int feature_params_resolve(const pt_feature_params *params, const pt_options *options, pt_feature_params *resolved);

// The denoiser's scratch buffers: one set per device, grown on demand, one call at a time per device.  They live as long as the process
// (never freed: a static destructor would run after the HIP runtime has gone).
struct DenoiseWorkspace {
    std::mutex mutex;
    size_t pixels = 0;  // capacity of the per-pixel buffers
    size_t staged = 0;  // ... and of the host form's upload/download buffers
    PtDenoiseScratch scratch{};
    float4 *in_rgba = nullptr, *in_features = nullptr;
    size_t staged_variance = 0; // ... and of pt_denoise_measured's upload buffer
    float4 *in_variance = nullptr;
};
DenoiseWorkspace &denoise_workspace(int device);
int denoise_ensure(DenoiseWorkspace &ws, size_t n, bool staged);
// The parameters pt_denoise takes (NULL = the defaults), checked without a device
int denoise_params_resolve(const pt_denoise_params *params, PtDenoiseParams *resolved);
// The same for pt_denoise_measured and pt_frame_preview_measured (NULL = pt_denoise_measured_params_default)
int denoise_measured_params_resolve(const pt_denoise_measured_params *params, PtDenoiseParams *resolved, float *sigma_measured);

} // namespace pth

#endif
