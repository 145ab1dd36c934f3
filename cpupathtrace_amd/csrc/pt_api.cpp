// pt_api.cpp -- host side of libpathtrace_hip.so: the C ABI of include/pt_hip.h.
//
// Scene creation flattens the caller's object list into the HBM layout of pt_types.h (building the reference's BVH
// topology on the way, pt_bvh.cpp / pt_build.hip); a render call is ONE launch of the persistent path kernel (pt_path.hip), whose
// wavefronts render the call's streams until none is left.  There is no CPU rendering path in this library.
#include "../../include/pt_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pt_build.h"
#include "pt_bvh.h"
#include "pt_kernels.h"
#include "pt_denoise.h"
#include "pt_post.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

#define PT_HIP(call)                                                                                               \
    do {                                                                                                           \
        hipError_t err_ = (call);                                                                                  \
        if(err_ != hipSuccess) {                                                                                   \
            return fail(PT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(err_));                          \
        }                                                                                                          \
    } while(0)

int env_int(const char *name, int fallback) {
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

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
float from_bits(uint32_t u) {
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

struct F4 {
    float x, y, z, w;
};

} // namespace

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
    std::vector<uint32_t> tri_obj;
    std::vector<uint32_t> sph_obj;
    uint32_t n_objects = 0;
    uint32_t n_emissive = 0;
    std::vector<int32_t> emissive_obj;
    std::vector<float> emissive_cdf;

    // device scene
    DevBuf<F4> recs, pairs, tris, tri_shade, spheres, materials, lights, emis; // (pairs and tris only while the scene is being built: linked into recs)
    DevBuf<uint2> sph_meta;
    DevBuf<float> emis_cdf;
    PtDevScene dev{};

    DevBuf<PtDevCounters> counters;
    DevBuf<F4> image;
    DevBuf<int4> tiles;
    DevBuf<uint32_t> tile_offset;
    DevBuf<float> batch_rays;

    // One render call at a time per scene: the workspace below is shared by every entry point (processItem may be called from several
    // threads on one const Scene, reference worker.h:66-69 / src/worker.cpp:328-362: such callers are serialised here).
    std::mutex render_mutex;

    // workspace of the persistent path kernel (pt_path.hip), grown on demand and reused between calls
    PtPathConfig path_cfg{};
    int path_blocks_per_cu = 0;
    uint32_t path_slots = 0, path_waves = 0, path_cap = 0;
    DevBuf<uint32_t> sl_nee_mask, pull_counter, tile_left;
    DevBuf<int4> st_rect;
    DevBuf<uint64_t> st_rng;
    DevBuf<F4> sl_state, sl_nee, lq_ray_o, lq_ray_d;
    DevBuf<PtEstimator> sl_est;
    DevBuf<PtCandidate> sl_cand;
    DevBuf<uint2> path_spill, closest_out;
    DevBuf<uint32_t> walk_save;
    DevBuf<PtPathArgs> path_args;  // the kernel's arguments in device memory
    PtPathArgs host_path_args{};   // ... and the host copy they are uploaded from
    DevBuf<unsigned long long> path_wave_counters;
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
    DevBuf<uint32_t> sl_cost, stream_cost, place;
    // a view batch (pt_render_views): the cameras and seeds of its views
    DevBuf<PtViewCamera> view_cams;
    DevBuf<uint64_t> view_seeds;
    // the first-hit features of a frame (pt_render_features*): the frame's features and the walks' spill area
    DevBuf<F4> features;
    DevBuf<uint2> feature_spill;
    DevBuf<PtViewCamera> feature_cams; // pt_render_features_views: the views' cameras, aperture none
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

namespace {

int device_count_quiet() {
    int n = 0;
    if(hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

PtDevCamera derive_camera(const pt_camera_params *c) {
    // Camera::Camera, src/camera.cpp:53-76
    PtDevCamera cam{};
    const Vec3 origin = ld(c->origin);
    const Vec3 forward_dir = normalize(sub(ld(c->look_at), origin));
    const Vec3 forward = scale(forward_dir, c->focal_length);
    const Vec3 up_dir = normalize(ld(c->up));
    const float height_half = c->height / 2.0F;
    const Vec3 up = scale(up_dir, height_half);
    const Vec3 right_dir = normalize(cross(forward, up));
    const float width_half = height_half * c->aspect_ratio;
    const Vec3 right = scale(right_dir, width_half);
    const Vec3 v[4] = {origin, forward, up, right};
    float *dst[4] = {cam.origin, cam.forward, cam.up, cam.right};
    for(int i = 0; i < 4; i++) {
        dst[i][0] = v[i].x;
        dst[i][1] = v[i].y;
        dst[i][2] = v[i].z;
    }
    cam.aperture_width_half = c->aperture_width / 2.0F;
    cam.aperture_height_half = c->aperture_height / 2.0F;
    cam.aperture_kind = c->aperture_kind;
    cam.hex_ratio = fmin_std(fmax_std(c->hex_ratio, 0.0F), 1.0F); // camera.cpp:22-24
    cam.focal_plane_dist = c->focal_plane_dist;
    return cam;
}

int derive_options(const pt_options *o, PtDevOptions *out) {
    PtDevOptions d{};
    d.image_width = o->image_width;
    d.image_height = o->image_height;
    d.min_sample_count = o->min_sample_count;
    d.max_sample_count = o->max_sample_count;
    d.overlap_bound = o->max_sample_count;
    d.epsilon = o->epsilon;
    d.pixel_width = 1.0F / static_cast<float>(o->image_width);
    d.pixel_height = 1.0F / static_cast<float>(o->image_height);
    // worker.cpp:158-164
    d.stats_sample_count = std::min(std::max(o->min_sample_count / 4, 1), 64);
    d.candidate_batch_count = std::max(std::max(o->min_sample_count, o->max_sample_count / 4) / d.stats_sample_count, 2);
    d.check_sample_count =
      std::min(std::max({o->min_sample_count / 2, (o->max_sample_count - o->min_sample_count) / 8, 8, d.stats_sample_count}), 1024) / d.stats_sample_count;
    // closed candidates a pixel can accumulate (worker.cpp:214-222).  A candidate closes after candidate_batch_count >= max / (4 S) batches
    // and a pixel has at most max / S of them, so at most 4 candidates ever close: the check below is a guard against a change of the
    // formulas above, not a limit a caller can reach (PT_MAX_CANDIDATES = 8).
    const int batches = std::max(o->max_sample_count, 0) / d.stats_sample_count;
    const int closed = batches > 0 ? (batches - 1) / d.candidate_batch_count : 0;
    if(closed > PT_MAX_CANDIDATES) {
        return fail(PT_ERR_UNSUPPORTED, "internal: the estimator's constants allow more than 8 closed candidates per pixel (worker.cpp:158-164 give at most 4)");
    }
    *out = d;
    return PT_OK;
}

int check_render_args(pt_scene *scene, const pt_camera_params *camera, const pt_options *options) {
    if(scene == nullptr || camera == nullptr || options == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(options->image_width <= 0 || options->image_height <= 0) {
        return fail(PT_ERR_INVALID, "image size must be positive");
    }
    return PT_OK;
}

// ---- the persistent path kernel (pt_path.hip): one launch per render call ---------------------------------------------------------------

struct Event {
    hipEvent_t e = nullptr;
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
    ~Event() {
        if(e != nullptr) {
            (void)hipEventDestroy(e);
        }
    }
};


int setup_path(pt_scene *s) {
    PtPathConfig &cfg = s->path_cfg;
    if(cfg.rows != 0) {
        return PT_OK;
    }
    cfg.in_lds = (s->dev.n_lds_pairs == s->dev.n_pairs && s->dev.n_lds_tris == s->dev.n_tris && s->dev.n_lds_pairs + s->dev.n_lds_tris > 0) ? 1 : 0;
    // 8 stack entries per lane in LDS (16 KB per workgroup) let four workgroups share a CU; deeper walks use the HBM spill area.  A scene
    // staged in LDS that leaves no room for four workgroups that way gets a window of 4 entries (pt_path.hip, PT_PATH_STACK_LDS_SMALL)
    cfg.wide = s->dev.n_lights + s->dev.n_object_samples > 8U ? 1 : 0;
    cfg.rows = std::min(std::max(env_int("PT_ROWS", 4), 1), PT_MAX_ROWS);
    cfg.stack_lds = pt_path_stack_lds(cfg.in_lds, pt_path_lds_bytes(cfg.wide, cfg.rows, 8, cfg.in_lds ? s->dev.n_lds_pairs : 0U, cfg.in_lds ? s->dev.pair_base : 0U));
    if(cfg.in_lds && env_int("PT_STACK_WINDOW", 0) > 0) {
        cfg.stack_lds = env_int("PT_STACK_WINDOW", 0) <= 4 ? 4 : 8; // (A/B: force the window of a scene in LDS)
    }
    cfg.lds_bytes = pt_path_lds_bytes(cfg.wide, cfg.rows, cfg.stack_lds, cfg.in_lds ? s->dev.n_lds_pairs : 0U, cfg.in_lds ? s->dev.pair_base : 0U);
    const int per_cu = pt_path_blocks_per_cu(cfg);
    const int limit = env_int("PT_BLOCKS_PER_CU", 0);
    s->path_blocks_per_cu = (limit > 0 && limit < per_cu) ? limit : per_cu;
    // a walk's stack holds at most one parked node per level of the tree and the sentinel at its bottom (pt_path.hip); what does not fit the LDS window spills
    cfg.spill_depth = s->depth + 2U > static_cast<uint32_t>(cfg.stack_lds) ? s->depth + 2U - static_cast<uint32_t>(cfg.stack_lds) : 1U;
    cfg.refill_idle = std::min(std::max(env_int("PT_REFILL_IDLE", 12), 1), 64);
    cfg.min_ready = std::min(std::max(env_int("PT_MIN_READY", 32), 1), 64 * PT_MAX_ROWS);
    cfg.ready_shift = std::min(std::max(env_int("PT_READY_SHIFT", 1), 0), 31);
    cfg.pass_q_low = std::max(env_int("PT_PASS_Q_LOW", 0), 0);
    cfg.early_ready = std::min(std::max(env_int("PT_EARLY_READY", 0), 0), 64 * PT_MAX_ROWS);
    cfg.compact_passes = env_int("PT_COMPACT", 1) != 0 ? 1 : 0;
    cfg.debug_lanes = std::min(std::max(env_int("PT_DEBUG_LANES", 64), 1), 64);
    // (burst_steps and leaf_min depend on the job's size as well: ensure_path_workspace sets them per job and keeps the last job's here)
    cfg.burst_steps = 24;
    cfg.leaf_min = 8;
    if(env_int("PT_DEBUG", 0) != 0) {
        std::fprintf(stderr, "[pt] path kernel: %d CUs x %d workgroups, %d rows of slots per wavefront, stack_lds %d, scene %s, lds %zu B, spill depth %u\n", s->cu_count,
                     s->path_blocks_per_cu, cfg.rows, cfg.stack_lds, cfg.in_lds ? "in LDS" : "in HBM", cfg.lds_bytes, cfg.spill_depth);
    }
    return PT_OK;
}

// A first round chosen by the host instead of the kernel's arithmetic: `waves` wavefronts (a multiple of 4) with `slots_per_wave` slots each,
// slot q of wavefront w starting with stream place[w * slots_per_wave + q] (device memory; 0xffffffff = the slot stays empty).
struct PathPlan {
    uint32_t waves = 0, slots_per_wave = 0;
    const uint32_t *d_place = nullptr;
};

// Grid and slot rows for n streams, and the buffers they need.
int ensure_path_workspace(pt_scene *s, uint32_t n, PtPathConfig *out_cfg, const PathPlan *plan = nullptr) {
    int rc = setup_path(s);
    if(rc != PT_OK) {
        return rc;
    }
    PtPathConfig cfg = s->path_cfg;
    const uint32_t max_grid = static_cast<uint32_t>(s->cu_count) * static_cast<uint32_t>(s->path_blocks_per_cu);
    // A stream's samples are sequential, so only more streams in flight shorten a job: a small job is spread over `spread` wavefronts
    // (a few per CU: enough to hide latency, few enough that a traversal step still serves many walks) before any wavefront gets a
    // full row of 64 slots; a large one fills the rows of every wavefront the chip holds.
    const uint32_t spread = std::min<uint32_t>(max_grid * 4U, static_cast<uint32_t>(std::max(env_int("PT_SPREAD_WAVES", 1024), 4)));
    uint32_t waves_wanted = (n + 63U) / 64U;                       // one row each
    if(waves_wanted < spread) {
        waves_wanted = std::min<uint32_t>(spread, n);              // thin rows
    }
    uint32_t grid = std::max<uint32_t>(1U, std::min<uint32_t>(max_grid, (waves_wanted + 3U) / 4U));
    if(plan != nullptr) {
        grid = std::max<uint32_t>(1U, std::min<uint32_t>(max_grid, plan->waves / 4U));
    }
    const uint32_t waves = grid * 4U;
    uint32_t slots_per_wave = std::min<uint32_t>(static_cast<uint32_t>(cfg.rows) * 64U, std::max<uint32_t>(1U, (n + waves - 1U) / waves));
    if(plan != nullptr) {
        if(waves != plan->waves || plan->slots_per_wave == 0 || plan->slots_per_wave > static_cast<uint32_t>(cfg.rows) * 64U) {
            return fail(PT_ERR_INVALID, "placement: " + std::to_string(plan->waves) + " wavefronts x " + std::to_string(plan->slots_per_wave) + " slots do not fit this device");
        }
        slots_per_wave = plan->slots_per_wave;
    }
    // The first round of streams goes to the slots in pieces of `first_lanes` neighbouring slots (pt_path.hip, stream hand-out): a
    // wavefront's slots are a whole number of pieces (a large job gets up to 7 more slots per wavefront, a small one pieces of 1).
    // A job that fits the slots in ONE round (nothing left to pull: every strong-scaling share of a frame, every small frame) has no
    // dynamic balance at all, and its duration is that of the wavefront with the most expensive streams -- whose samples are sequential, so
    // the streams that happen to share a wavefront with them wait for the same passes.  Such a job is dealt stream by stream (pieces of 1:
    // slot q of wavefront w renders stream q * waves + w), which gives every wavefront a sample of the whole job: the 1/8 share of the
    // benchmark frame 273 -> 221 ms at 256 spp, the 1/4 share 317 -> 259 (profiles/r03_share_rehearsal.txt).
    const bool single_round = plan != nullptr || (static_cast<uint64_t>(waves) * slots_per_wave >= n && slots_per_wave <= 128U); // (a full grid of 4 rows balances well in pieces of 8: 423 against 409 Msamples/s)
    uint32_t first_lanes = plan != nullptr ? 1U : static_cast<uint32_t>(env_int("PT_FIRST_LANES", single_round ? 1 : 8)); // full frame: 64 -> 402, 32 -> 403, 16 -> 434, 8 -> 440, 4 -> 431 Msamples/s
    if(first_lanes == 0 || first_lanes > 64 || (first_lanes & (first_lanes - 1U)) != 0) {
        first_lanes = single_round ? 1 : 8;
    }
    if(slots_per_wave % first_lanes != 0) {
        if(slots_per_wave >= 64U) {
            slots_per_wave = (slots_per_wave + first_lanes - 1U) / first_lanes * first_lanes; // (rows * 64 is a multiple of every piece size)
        }
        else {
            first_lanes = 1;
        }
    }
    cfg.first_lanes = static_cast<int>(first_lanes);
    // Steps between two looks at the ring.  Trees in HBM: 8 -> 397, 12 -> 407, 16 -> 412, 24 -> 422, 32 -> 421 Msamples/s on the benchmark frame
    // (round 3 made the step cheaper, looking at the ring costs what it did); scenes in LDS keep 12 on a full grid (Cornell: 700 against 659
    // with 24) and take 24 when a wavefront has less than a row of slots (the reference's benchmark program, 128 x 128: 136 -> 176 Msamples/s).
    // Shallower trees in HBM have shorter walks, and looking at the ring more often pays again (profiles/r03_tree_size_knobs.txt): 160-330
    // triangles (10, 11 levels) 12 -> 795 / 764 against 788 / 756 with 24; 3 K (14 levels) 16 -> 662 against 610 (one and two rows of slots:
    // 522 against 502, 621 against 575); 20 K (17 levels) 16 -> 589 against 564; from 180 K (22 levels) on 24 wins.  Scenes in LDS: 12 with
    // several rows of slots (Cornell 1024 x 1024: 700 against 659, 724 x 724: 656 against 635), 24 with one (256 x 256: 221 against 218, Box 406 against 373).
    int burst_default = 24;
    if(cfg.in_lds) {
        burst_default = slots_per_wave > 64U ? 12 : 24;
    }
    else if(slots_per_wave >= 64U) {
        burst_default = s->depth <= 12U ? 12 : (s->depth <= 18U ? 16 : 24);
    }
    cfg.burst_steps = std::min(std::max(env_int("PT_BURST", burst_default), 1), 64);
    // Lanes that wait for the rare step (leaves) before it runs: 2 -> 374, 4 -> 396, 8 -> 414, 12 -> 415 Msamples/s on the benchmark frame; a
    // wavefront with 16 slots cannot wait for 8 of them (128 x 128, 180 k triangles: 8 -> 54, 4 -> 59, 2 -> 62 Msamples/s)
    // Scenes in LDS (a leaf test is a larger share of a walk of 7-10 nodes): 8 -> 685 / 1160, 16 -> 724 / 1201, 24 -> 729 / 1193, 32 -> 707 / 1189 Msamples/s on
    // Cornell / Box with full rows (profiles/r03_lds_scene_knobs.txt); wavefronts with less than a row of slots keep 8
    // trees in HBM of up to 24 levels (720 K triangles) with full rows: 12 instead of 8 brings 1-4 % (3 K triangles 599 -> 610, 20 K 552 -> 564, 180 K 523 -> 530,
    // 720 K 483 -> 488); the benchmark's 30 levels keep 8 (430 against 425)
    int leaf_default = cfg.in_lds ? (slots_per_wave >= 64U ? 16 : 8) : static_cast<int>(std::min<uint32_t>(std::max<uint32_t>(slots_per_wave / 8U, 2U), 8U));
    if(!cfg.in_lds && slots_per_wave >= 64U && s->depth <= 24U) {
        leaf_default = 12;
    }
    cfg.leaf_min = std::min(std::max(env_int("PT_LEAF_MIN", leaf_default), 1), 64);
    const uint32_t rows = (slots_per_wave + 63U) / 64U;
    const uint32_t total = waves * rows * 64U;
    const uint32_t rays_per_slot = 1U + s->dev.n_lights + s->dev.n_object_samples;
    uint32_t cap = rows * 64U * rays_per_slot;
    const int ring_log = env_int("PT_RING_LOG_RAYS", 0); // diagnostic: rings that never wrap keep every ray of the frame (pt_debug_replay_rays)
    if(ring_log > 0) {
        cap = std::max<uint32_t>(cap, static_cast<uint32_t>(ring_log));
    }
    cfg.grid = static_cast<int>(grid);
    cfg.rows = static_cast<int>(rows);
    cfg.slots_per_wave = static_cast<int>(slots_per_wave);
    // (the kernel addresses the slot state with 32-bit byte offsets)
    if(static_cast<unsigned long long>(total) * PT_SLOT_PLANES * sizeof(F4) > 0xffffffffULL) {
        return fail(PT_ERR_UNSUPPORTED, "path kernel: " + std::to_string(total) + " slots do not fit the 4 GiB the slot state may occupy");
    }
    PT_HIP(s->sl_state.ensure(static_cast<size_t>(total) * PT_SLOT_PLANES));
    PT_HIP(s->sl_nee.ensure(static_cast<size_t>(total) * std::max<uint32_t>(rays_per_slot - 1U, 1U)));
    PT_HIP(s->sl_nee_mask.ensure(total));
    PT_HIP(s->sl_cost.ensure(total));
    PT_HIP(s->sl_est.ensure(total));
    PT_HIP(s->sl_cand.ensure(static_cast<size_t>(total) * PT_MAX_CANDIDATES));
    PT_HIP(s->lq_ray_o.ensure(static_cast<size_t>(waves) * cap));
    PT_HIP(s->lq_ray_d.ensure(static_cast<size_t>(waves) * cap));
    if(ring_log > 0) {
        PT_HIP(hipMemsetAsync(s->lq_ray_d.ptr, 0xff, static_cast<size_t>(waves) * cap * 4 * sizeof(float), s->stream));
    }
    PT_HIP(s->path_spill.ensure(static_cast<size_t>(waves) * 64U * cfg.spill_depth));
    PT_HIP(s->path_wave_counters.ensure(static_cast<size_t>(waves) * 8U));
    PT_HIP(s->walk_save.ensure(static_cast<size_t>(waves) * 64U * PT_WALK_SAVE_WORDS));
    PT_HIP(s->pull_counter.ensure(64));
    PT_HIP(s->counters.ensure(1));
    cfg.spill = s->path_spill.ptr;
    cfg.walk_save = s->walk_save.ptr;
    cfg.wave_counters = s->path_wave_counters.ptr;
    s->path_slots = total;
    s->path_waves = waves;
    s->path_cap = cap;
    s->path_cfg.burst_steps = cfg.burst_steps; // (the diagnostics that follow a render -- pt_debug_replay_rays -- run with its settings)
    s->path_cfg.leaf_min = cfg.leaf_min;
    *out_cfg = cfg;
    return PT_OK;
}

// The stop of one controlled call (pt_render_tiles_ctl), shared by the host threads of its replicas.  The stop travels to the device as
// one word per replica in pinned, fine-grained host memory; the host loop of every launch polls the caller's cancel flag and the deadline,
// and the first one to see either writes 1 into the word of every replica whose launch is prepared or running.
struct RenderStop {
    typedef std::chrono::steady_clock Clock;
    pt_render_control *ctl = nullptr;
    bool has_deadline = false;
    Clock::time_point deadline;
    std::atomic<bool> requested{false};
    std::mutex mutex; // guards what follows
    Clock::time_point requested_at;
    std::vector<uint32_t *> words; // the cancel words of the launches prepared or running
    double drain_ms = 0.0;         // the latest end of a launch after the request

    // a launch takes part: its word starts as the stop's state (a request that came before the launch stops it at its first pass)
    void enlist(uint32_t *word) {
        std::lock_guard<std::mutex> lock(mutex);
        __atomic_store_n(word, requested.load() ? 1U : 0U, __ATOMIC_SEQ_CST);
        words.push_back(word);
    }
    // ... and has ended (seen by its host loop at `end`): its word may serve another call now
    void retire(uint32_t *word, Clock::time_point end) {
        std::lock_guard<std::mutex> lock(mutex);
        words.erase(std::remove(words.begin(), words.end(), word), words.end());
        if(requested.load()) {
            drain_ms = std::max(drain_ms, std::chrono::duration<double, std::milli>(end - requested_at).count());
        }
    }
    void poll() {
        if(requested.load(std::memory_order_relaxed)) {
            return;
        }
        const Clock::time_point now = Clock::now();
        if(__atomic_load_n(&ctl->cancel, __ATOMIC_ACQUIRE) == 0 && !(has_deadline && now >= deadline)) {
            return;
        }
        std::lock_guard<std::mutex> lock(mutex);
        if(!requested.load()) {
            requested_at = now;
            requested.store(true);
            for(uint32_t *w : words) {
                __atomic_store_n(w, 1U, __ATOMIC_SEQ_CST);
            }
        }
    }
};

// Streams of a launch that no wavefront took: the first round (streams 0 .. first_total-1) is always dealt out, beyond it the final value
// of the pull counter says how many were handed out (it may overshoot the job: a wavefront's last pull asks for a whole row)
uint64_t unclaimed_streams(uint64_t n, uint64_t first_total, uint64_t pulled) {
    const uint64_t first = std::min(n, first_total);
    return n - first - std::min(pulled, n - first);
}

// What a controlled launch did with its streams (finish_path)
struct StreamTally {
    uint64_t finished = 0, abandoned = 0, unclaimed = 0;
};

// Wait for the scene's stream and make sure the last launch rendered every stream it was given: a wavefront that left early or a stream
// lost in the hand-out would otherwise return stale pixels with PT_OK.  Every entry point that synchronises anyway ends with this.  A
// controlled launch must account for every stream as finished, abandoned or never taken; `tally` (may be null) receives the three.
int finish_path(pt_scene *s, StreamTally *tally = nullptr) {
    PT_HIP(hipStreamSynchronize(s->stream));
    if(s->host_streams_done != nullptr && s->streams_expected != 0) {
        const volatile unsigned long long *h = static_cast<volatile unsigned long long *>(s->host_streams_done);
        const unsigned long long done = h[0];
        const uint64_t expected = s->streams_expected;
        s->streams_expected = 0;
        if(s->streams_controlled) {
            s->streams_controlled = false;
            StreamTally t;
            t.finished = done;
            t.abandoned = h[1];
            t.unclaimed = unclaimed_streams(expected, s->streams_first_total, static_cast<uint32_t>(h[2]));
            if(t.finished + t.abandoned + t.unclaimed != expected) {
                return fail(PT_ERR_HIP, "path kernel ended with " + std::to_string(t.finished) + " finished, " + std::to_string(t.abandoned) + " abandoned and " +
                                            std::to_string(t.unclaimed) + " unclaimed of " + std::to_string(expected) + " streams");
            }
            if(tally != nullptr) {
                *tally = t;
            }
        }
        else if(done != expected) {
            return fail(PT_ERR_HIP, "path kernel ended with " + std::to_string(done) + " of " + std::to_string(expected) + " streams finished");
        }
    }
    return PT_OK;
}

// Render the streams described by T (device pointers) with one launch on the scene's stream.  With a progress function the host polls
// the count of finished tiles (pinned memory, written by the kernel) while the launch runs and reports every step from the calling thread.
// With a RenderStop (controlled launches) the host loop runs whether or not there is a progress function: it forwards a stop request to the
// launch through the scene's cancel word.
int run_path(pt_scene *s, const PtDevCamera &cam, const PtDevOptions &opt, PtStreams T, float4 *d_image, pt_stats *stats, pt_progress_fn progress, void *progress_user,
             const PathPlan *plan = nullptr, bool want_costs = false, RenderStop *stop = nullptr) {
    PtPathConfig cfg;
    hipStream_t st = s->stream;
    PathPlan debug_plan;
    if(plan == nullptr && !s->debug_place.empty()) {
        // pt_debug_set_place: this launch only
        PT_HIP(s->place.ensure(s->debug_place.size()));
        PT_HIP(hipMemcpyAsync(s->place.ptr, s->debug_place.data(), s->debug_place.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        PT_HIP(hipStreamSynchronize(st));
        debug_plan.waves = s->debug_place_waves;
        debug_plan.slots_per_wave = s->debug_place_slots;
        debug_plan.d_place = s->place.ptr;
        s->debug_place.clear();
        plan = &debug_plan;
    }
    int rc = ensure_path_workspace(s, T.n, &cfg, plan);
    if(rc != PT_OK) {
        return rc;
    }
    want_costs = want_costs || s->debug_collect_costs;
    T.place = plan != nullptr ? plan->d_place : nullptr;
    T.cost = nullptr;
    if(want_costs) {
        PT_HIP(s->stream_cost.ensure(std::max<uint32_t>(T.n, 1U)));
        T.cost = s->stream_cost.ptr;
    }
    PtSlots S{};
    S.total = s->path_slots;
    S.state = reinterpret_cast<float4 *>(s->sl_state.ptr);
    S.nee = reinterpret_cast<float4 *>(s->sl_nee.ptr);
    S.nee_mask = s->sl_nee_mask.ptr;
    S.cost = s->sl_cost.ptr;
    S.est = s->sl_est.ptr;
    S.cand = s->sl_cand.ptr;
    PtLocalQueue Q{};
    Q.ray_o = reinterpret_cast<float4 *>(s->lq_ray_o.ptr);
    Q.ray_d = reinterpret_cast<float4 *>(s->lq_ray_d.ptr);
    Q.cap = s->path_cap;
    T.next = s->pull_counter.ptr;
    T.first_total = plan != nullptr ? T.n : s->path_waves * static_cast<uint32_t>(cfg.slots_per_wave); // (a placement names every stream: nothing is left to pull)
    T.n_waves = s->path_waves;
    // The first round (pt_path.hip, stream hand-out): piece q of wavefront w -- `first_lanes` neighbouring slots -- starts on the chunk
    // q * waves + w of as many streams, moved q steps sideways in a regular tile grid.
    T.first_spread = env_int("PT_FIRST_SPREAD", 1) != 0 ? 1U : 0U;
    T.first_lanes = static_cast<uint32_t>(cfg.first_lanes);
    T.first_shift = static_cast<uint32_t>(std::max(env_int("PT_FIRST_SHIFT", 1), 0));
    {
        // the sideways move needs: a regular grid, a first round that does not reach beyond the job and covers whole grid rows per piece,
        // and as many tiles per grid row as a multiple of the pieces of a wavefront
        const uint32_t pieces = static_cast<uint32_t>(cfg.slots_per_wave) / T.first_lanes;
        const unsigned long long per_grid_row = static_cast<unsigned long long>(T.chunks_per_tile) * (64U / T.first_lanes) * T.tiles_per_row;
        if(env_int("PT_FIRST_SPREAD", 1) == 2 || per_grid_row == 0 || s->path_waves % per_grid_row != 0 || T.first_total > T.n || (T.tiles_per_row % pieces != 0 && pieces % T.tiles_per_row != 0)) {
            T.tiles_per_row = 0;
        }
    }
    uint32_t *const own_left = T.tile_left; // (a resumable frame keeps its own count of pixels per tile from launch to launch)
    T.tile_left = nullptr;
    T.tiles_done = nullptr;
    T.cancel = nullptr;
    if((progress != nullptr || stop != nullptr) && T.rect == nullptr && T.n_tiles > 0) {
        if(s->host_tiles_done == nullptr) {
            PT_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->host_tiles_done), 64, hipHostMallocDefault));
        }
        *s->host_tiles_done = 0;
        T.tiles_done = s->host_tiles_done;
        T.tile_left = own_left != nullptr ? own_left : s->tile_left.ptr; // filled by the caller (pixels per tile)
    }
    PT_HIP(hipMemsetAsync(s->counters.ptr, 0, sizeof(PtDevCounters), st));
    PT_HIP(hipMemsetAsync(s->pull_counter.ptr, 0, 64 * sizeof(uint32_t), st));
    PT_HIP(hipMemsetAsync(s->path_wave_counters.ptr, 0, static_cast<size_t>(s->path_waves) * 8U * sizeof(unsigned long long), st));
    Event ev_begin, ev_end;
    PT_HIP(ev_begin.create());
    PT_HIP(ev_end.create());
    PT_HIP(hipEventRecord(ev_begin.e, st));
    PT_HIP(s->path_args.ensure(1));
    if(stop != nullptr) {
        if(s->host_cancel == nullptr) {
            // coherent (fine-grained): the device must not keep a cached copy of the word for the length of the launch
            PT_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->host_cancel), 64, hipHostMallocCoherent | hipHostMallocMapped));
            PT_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&s->dev_cancel), s->host_cancel, 0));
        }
        T.cancel = s->dev_cancel;
    }
    // (from here until the host loop has seen the launch end, a stop request reaches this launch)
    struct Enlisted {
        RenderStop *stop;
        uint32_t *word;
        ~Enlisted() {
            if(stop != nullptr) {
                stop->retire(word, RenderStop::Clock::now());
            }
        }
    } enlisted{stop, s->host_cancel};
    if(stop != nullptr) {
        stop->enlist(s->host_cancel);
    }
    pt_launch_path(st, s->dev, cam, opt, S, T, Q, cfg, d_image, s->counters.ptr, &s->host_path_args, s->path_args.ptr);
    PT_HIP(hipGetLastError());
    PT_HIP(hipEventRecord(ev_end.e, st));
    // every launch leaves its count of finished streams in pinned memory; whoever waits for the stream next compares it (finish_path)
    if(s->host_streams_done == nullptr) {
        PT_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->host_streams_done), 64, hipHostMallocDefault));
    }
    *s->host_streams_done = ~0ULL;
    s->streams_expected = T.n;
    PT_HIP(hipMemcpyAsync(s->host_streams_done, &s->counters.ptr->streams_done, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    s->streams_controlled = stop != nullptr;
    if(stop != nullptr) {
        s->host_streams_done[1] = ~0ULL;
        s->host_streams_done[2] = ~0ULL;
        s->streams_first_total = T.first_total;
        PT_HIP(hipMemcpyAsync(s->host_streams_done + 1, &s->counters.ptr->streams_abandoned, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        PT_HIP(hipMemcpyAsync(s->host_streams_done + 2, s->pull_counter.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    if(T.tiles_done != nullptr) {
        const int total = static_cast<int>(T.n_tiles);
        int reported = 0;
        for(;;) {
            const hipError_t q = hipEventQuery(ev_end.e);
            const int done = std::min(static_cast<int>(*static_cast<volatile uint32_t *>(s->host_tiles_done)), total);
            while(progress != nullptr && reported < done) {
                progress(++reported, total, progress_user);
            }
            if(q == hipSuccess) {
                break;
            }
            if(q != hipErrorNotReady) {
                return fail(PT_ERR_HIP, std::string("path kernel: ") + hipGetErrorString(q));
            }
            if(stop != nullptr) {
                stop->poll(); // (after the callback: a cancel from it reaches the device at once)
            }
            std::this_thread::sleep_for(std::chrono::microseconds(500));
        }
        if(stop != nullptr) {
            stop->retire(s->host_cancel, RenderStop::Clock::now());
            enlisted.stop = nullptr;
        }
        const int done = std::min(static_cast<int>(*static_cast<volatile uint32_t *>(s->host_tiles_done)), total);
        while(progress != nullptr && reported < done) {
            progress(++reported, total, progress_user);
        }
    }
    if(stats != nullptr) {
        PT_HIP(hipEventSynchronize(ev_end.e));
        float ms = 0.0F;
        PT_HIP(hipEventElapsedTime(&ms, ev_begin.e, ev_end.e));
        std::vector<unsigned long long> slots(static_cast<size_t>(s->path_waves) * 8U);
        PT_HIP(hipMemcpy(slots.data(), s->path_wave_counters.ptr, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, kcycles[3] = {0, 0, 0};
        for(size_t i = 0; i < slots.size(); i++) {
            // (a PT_PATH_TIMING build packs kilo-cycle totals into the high words of three slots; they are zero otherwise)
            const size_t k = i & 7U;
            sum[k] += (k >= 3 && k <= 5) ? (slots[i] & 0xffffffffULL) : slots[i];
            if(k >= 3 && k <= 5) {
                kcycles[k - 3] += slots[i] >> 32;
            }
        }
        if(kcycles[0] != 0 && env_int("PT_DEBUG", 0) != 0) {
            std::fprintf(stderr, "[pt] wave time: %.1f %% in shading passes, %.1f %% in traversal bursts (of the waves' lifetimes; %llu kilo-cycles in all)\n",
                         100.0 * static_cast<double>(kcycles[2]) / static_cast<double>(kcycles[0]), 100.0 * static_cast<double>(kcycles[1]) / static_cast<double>(kcycles[0]), kcycles[0]);
        }
        PtDevCounters done{};
        PT_HIP(hipMemcpy(&done, s->counters.ptr, sizeof(done), hipMemcpyDeviceToHost));
        if(stop != nullptr) {
            uint32_t pulled = 0;
            PT_HIP(hipMemcpy(&pulled, s->pull_counter.ptr, sizeof(pulled), hipMemcpyDeviceToHost));
            const uint64_t unclaimed = unclaimed_streams(T.n, T.first_total, pulled);
            if(done.streams_done + done.streams_abandoned + unclaimed != T.n) {
                return fail(PT_ERR_HIP, "path kernel ended with " + std::to_string(done.streams_done) + " finished, " + std::to_string(done.streams_abandoned) + " abandoned and " +
                                            std::to_string(unclaimed) + " unclaimed of " + std::to_string(T.n) + " streams");
            }
        }
        else if(done.streams_done != T.n) {
            return fail(PT_ERR_HIP, "path kernel ended with " + std::to_string(done.streams_done) + " of " + std::to_string(T.n) + " streams finished");
        }
        stats->node_visits = sum[0];
        stats->leaf_tests = sum[1];
        stats->rays_traced = sum[2];
        stats->shadow_rays_traced = sum[3];
        stats->samples = sum[6];
        stats->vertices = sum[7];
        stats->launches = 1;
        stats->kernel_ms = ms;
        stats->wave_steps = sum[4];
        stats->shading_passes = sum[5];
        stats->wavefronts = s->path_waves;
        stats->slot_rows = static_cast<uint64_t>(cfg.rows);
        if(env_int("PT_DEBUG", 0) != 0) {
            std::fprintf(stderr, "[pt] path kernel: %.2f ms, grid %d x 256, %d rows; wave steps %llu (%.1f lanes of 64 busy per step), shading passes %llu, rays %llu\n", ms, cfg.grid,
                         cfg.rows, sum[4], sum[4] ? static_cast<double>(sum[0] + sum[1]) / static_cast<double>(sum[4]) : 0.0, sum[5], sum[2]);
            // balance: a wavefront's busy time follows its steps; the launch lasts as long as the busiest one
            std::vector<unsigned long long> steps(s->path_waves);
            for(size_t w = 0; w < steps.size(); w++) {
                steps[w] = slots[8 * w + 4] & 0xffffffffULL;
            }
            std::sort(steps.begin(), steps.end());
            const double mean = static_cast<double>(sum[4]) / static_cast<double>(steps.size());
            std::fprintf(stderr, "[pt] wave steps per wavefront: mean %.0f, min %llu, median %llu, 90 %% %llu, 99 %% %llu, max %llu (max / mean %.3f)\n", mean, steps.front(),
                         steps[steps.size() / 2], steps[steps.size() * 9 / 10], steps[steps.size() * 99 / 100], steps.back(), static_cast<double>(steps.back()) / mean);
        }
    }
    return PT_OK;
}

} // namespace

extern "C" {

int pt_device_count(void) {
    return device_count_quiet();
}

const char *pt_last_error(void) {
    return g_last_error.c_str();
}

uint64_t pt_pixel_seed(uint64_t base_seed, int32_t x, int32_t y) {
    // splitmix64 finaliser over (base_seed, x, y); the device computes the same (pt_shading.h pixel_seed)
    uint64_t z = base_seed + 0x9E3779B97F4A7C15ULL * (1ULL + (static_cast<uint64_t>(static_cast<uint32_t>(y)) << 32) + static_cast<uint64_t>(static_cast<uint32_t>(x)));
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

uint64_t pt_rng_seed_to_state(uint64_t seed) {
    return seed ^ (~seed << 32);
}

size_t pt_job_tiles(int32_t image_width, int32_t image_height, pt_tile *out, size_t capacity) {
    // processJob, src/worker.cpp:389-414
    const int width = std::max(image_width, 0);
    const int height = std::max(image_height, 0);
    if(width == 0 || height == 0) {
        return 0;
    }
    const int tile_size = std::max(std::min(std::min(width, height) / 4, 32), 1);
    const int horizontal_tiles = (width + (tile_size - 1)) / tile_size;
    const int vertical_tiles = (height + (tile_size - 1)) / tile_size;
    size_t n = 0;
    for(int ty = 0; ty < vertical_tiles; ty++) {
        for(int tx = 0; tx < horizontal_tiles; tx++) {
            if(out != nullptr && n < capacity) {
                const int ox = tx * tile_size, oy = ty * tile_size;
                out[n] = pt_tile{ox, oy, std::min(width - ox, tile_size), std::min(height - oy, tile_size)};
            }
            n++;
        }
    }
    return n;
}

int pt_scene_create(int device, const pt_scene_desc *d, pt_scene **out) {
    if(d == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    *out = nullptr;
    const int n_dev = device_count_quiet();
    if(n_dev <= 0) {
        return fail(PT_ERR_NO_DEVICE, "no HIP device available; libpathtrace_hip has no CPU path");
    }
    if(device < 0 || device >= n_dev) {
        return fail(PT_ERR_NO_DEVICE, "device index out of range");
    }
    if(d->n_objects != d->n_triangles + d->n_spheres) {
        return fail(PT_ERR_INVALID, "n_objects must equal n_triangles + n_spheres");
    }
    if((d->n_objects > 0 && d->obj_kind == nullptr) || (d->n_triangles > 0 && (d->tri_pos == nullptr || d->tri_cull == nullptr || d->tri_material == nullptr)) ||
       (d->n_spheres > 0 && (d->sph == nullptr || d->sph_material == nullptr)) || (d->n_materials > 0 && d->materials == nullptr) ||
       (d->n_point_lights > 0 && (d->light_pos == nullptr || d->light_spectrum == nullptr))) {
        return fail(PT_ERR_INVALID, "missing array in scene description");
    }
    if(d->n_triangles > PT_REF_INDEX || d->n_spheres > PT_REF_INDEX) {
        return fail(PT_ERR_UNSUPPORTED, "too many objects");
    }

    std::unique_ptr<pt_scene> s(new pt_scene());
    s->device = device;
    PT_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    PT_HIP(hipGetDeviceProperties(&prop, device));
    s->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    PT_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->n_objects = d->n_objects;

    using clock = std::chrono::steady_clock;
    const auto t_begin = clock::now();
    auto ms_since = [](clock::time_point t0) { return std::chrono::duration<float, std::milli>(clock::now() - t0).count(); };

    // ---- objects in construction order: typed indices and the reference word of every leaf ---------------------------------
    std::vector<uint32_t> leaf_ref(d->n_objects);
    s->tri_obj.resize(d->n_triangles);
    s->sph_obj.resize(d->n_spheres);
    {
        uint32_t ti = 0, si = 0;
        for(uint32_t i = 0; i < d->n_objects; i++) {
            if(d->obj_kind[i] == PT_OBJ_TRIANGLE) {
                if(ti >= d->n_triangles) {
                    return fail(PT_ERR_INVALID, "obj_kind lists more triangles than n_triangles");
                }
                leaf_ref[i] = PT_REF_LEAF | ti;
                s->tri_obj[ti] = i;
                if(d->tri_material[ti] != PT_NO_MATERIAL && d->tri_material[ti] >= d->n_materials) {
                    return fail(PT_ERR_INVALID, "triangle material index out of range");
                }
                ti++;
            }
            else if(d->obj_kind[i] == PT_OBJ_SPHERE) {
                if(si >= d->n_spheres) {
                    return fail(PT_ERR_INVALID, "obj_kind lists more spheres than n_spheres");
                }
                leaf_ref[i] = PT_REF_LEAF | PT_REF_SPHERE | si;
                s->sph_obj[si] = i;
                if(d->sph_material[si] != PT_NO_MATERIAL && d->sph_material[si] >= d->n_materials) {
                    return fail(PT_ERR_INVALID, "sphere material index out of range");
                }
                si++;
            }
            else {
                return fail(PT_ERR_INVALID, "unknown object kind");
            }
        }
    }
    s->n_nodes = d->n_objects > 0 ? 2ULL * d->n_objects - 1ULL : 0ULL;

    // Where the tree is built.  PT_BUILD=device | host forces one; by default scenes of 1024 objects or more are built on the
    // device (pt_build.hip) and smaller ones by the host recursion (pt_bvh.cpp).  Both produce the same arrays, bit for bit.
    bool use_device = d->n_objects >= static_cast<uint32_t>(std::max(env_int("PT_BUILD_DEVICE_MIN", 1024), 2));
    if(const char *mode = std::getenv("PT_BUILD")) {
        if(std::strcmp(mode, "host") == 0) {
            use_device = false;
        }
        else if(std::strcmp(mode, "device") == 0) {
            use_device = d->n_objects >= 2;
        }
    }
    s->device_built = use_device;
    const bool align_siblings = env_int("PT_ALIGN_SIBLINGS", 1) != 0;

    std::vector<int32_t> dfs; // leaves depth-first, left to right (Scene::registerEmissiveObjects order); device path: only those with an emissive material
    uint32_t n_pairs = 0, root_ref = PT_REF_NONE;
    float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};
    if(use_device) {
        // ---- device: upload the caller's arrays as they are; records, leaf boxes and the tree are made in HBM ----------------------
        s->build_ms[0] = ms_since(t_begin);
        const auto t_upload = clock::now();
        DevBuf<float> raw_pos, raw_nrm, raw_sph;
        DevBuf<uint8_t> raw_cull;
        DevBuf<uint32_t> raw_tri_mat, raw_tri_obj, raw_sph_mat, raw_sph_obj;
        auto up = [](auto &buf, const auto *src, size_t count) -> hipError_t {
            hipError_t e = buf.ensure(count);
            if(e != hipSuccess || count == 0) {
                return e;
            }
            return hipMemcpy(buf.ptr, src, count * sizeof(*src), hipMemcpyHostToDevice);
        };
        PT_HIP(up(raw_pos, d->tri_pos, 9 * static_cast<size_t>(d->n_triangles)));
        if(d->tri_nrm != nullptr) {
            PT_HIP(up(raw_nrm, d->tri_nrm, 9 * static_cast<size_t>(d->n_triangles)));
        }
        PT_HIP(up(raw_cull, d->tri_cull, d->n_triangles));
        PT_HIP(up(raw_tri_mat, d->tri_material, d->n_triangles));
        PT_HIP(up(raw_tri_obj, s->tri_obj.data(), d->n_triangles));
        PT_HIP(up(raw_sph, d->sph, 4 * static_cast<size_t>(d->n_spheres)));
        PT_HIP(up(raw_sph_mat, d->sph_material, d->n_spheres));
        PT_HIP(up(raw_sph_obj, s->sph_obj.data(), d->n_spheres));
        PT_HIP(s->tris.ensure(PT_TRI_QUADS * (static_cast<size_t>(d->n_triangles) + 1 + d->n_spheres))); // triangles, a spare record, spheres (pt_types.h)
        PT_HIP(hipMemsetAsync(s->tris.ptr + PT_TRI_QUADS * static_cast<size_t>(d->n_triangles), 0, PT_TRI_QUADS * sizeof(F4), s->stream));
        PT_HIP(s->tri_shade.ensure(8 * static_cast<size_t>(d->n_triangles)));
        PT_HIP(s->spheres.ensure(d->n_spheres));
        PT_HIP(s->sph_meta.ensure(d->n_spheres));
        s->build_ms[1] = ms_since(t_upload);

        PtBuildInput in;
        in.n_objects = d->n_objects;
        in.n_triangles = d->n_triangles;
        in.n_spheres = d->n_spheres;
        in.tri_pos = raw_pos.ptr;
        in.tri_nrm = d->tri_nrm != nullptr ? raw_nrm.ptr : nullptr;
        in.tri_cull = raw_cull.ptr;
        in.tri_material = raw_tri_mat.ptr;
        in.tri_obj = raw_tri_obj.ptr;
        in.sph = raw_sph.ptr;
        in.sph_material = raw_sph_mat.ptr;
        in.sph_obj = raw_sph_obj.ptr;
        in.align_siblings = align_siblings;
        PtBuildOutput built;
        built.tris = reinterpret_cast<float4 *>(s->tris.ptr);
        built.tri_shade = reinterpret_cast<float4 *>(s->tri_shade.ptr);
        built.spheres = reinterpret_cast<float4 *>(s->spheres.ptr);
        built.sph_meta = s->sph_meta.ptr;
        const char *what = "";
        const hipError_t e = pt_build_scene_device(s->stream, in, built, &what);
        if(e != hipSuccess) {
            return fail(PT_ERR_HIP, std::string("device scene build (") + what + "): " + hipGetErrorString(e));
        }
        s->pairs.ptr = reinterpret_cast<F4 *>(built.pairs);
        s->pairs.count = 4 * static_cast<size_t>(built.n_pairs);
        DevBuf<uint32_t> dfs_dev;
        dfs_dev.ptr = built.dfs;
        dfs_dev.count = d->n_objects;
        s->build_ms[2] = built.build_ms;
        s->depth = built.depth;
        if(s->depth > PT_MAX_DEPTH) {
            return fail(PT_ERR_UNSUPPORTED, "internal: BVH deeper than 128 levels (impl::constructBVH keeps a child at two thirds of its parent at most: 53 levels for 2^30 objects; tests/test_oracle_golden.py)");
        }
        n_pairs = built.n_pairs;
        root_ref = built.root_ref;
        for(int k = 0; k < 3; k++) {
            root_lo[k] = built.root_lo[k];
            root_hi[k] = built.root_hi[k];
        }
        // Only objects with an emissive material matter to registerEmissiveObjects: pick them out in construction order on the
        // host (sequential reads) and let the device put them into depth-first order.
        std::vector<uint8_t> lit(d->n_materials, 0);
        bool any_lit = false;
        for(uint32_t m = 0; m < d->n_materials; m++) {
            const float *e = d->materials[m].emission;
            lit[m] = (e[0] + e[1] + e[2]) * e[3] > 0.0F ? 1 : 0;
            any_lit = any_lit || lit[m] != 0;
        }
        if(any_lit) {
            std::vector<uint32_t> mask((static_cast<size_t>(d->n_objects) + 31) / 32, 0U);
            uint32_t n_selected = 0;
            for(uint32_t t = 0; t < d->n_triangles; t++) {
                const uint32_t m = d->tri_material[t];
                if(m != PT_NO_MATERIAL && lit[m] != 0) {
                    const uint32_t o = s->tri_obj[t];
                    mask[o >> 5] |= 1U << (o & 31U);
                    n_selected++;
                }
            }
            for(uint32_t i = 0; i < d->n_spheres; i++) {
                const uint32_t m = d->sph_material[i];
                if(m != PT_NO_MATERIAL && lit[m] != 0) {
                    const uint32_t o = s->sph_obj[i];
                    mask[o >> 5] |= 1U << (o & 31U);
                    n_selected++;
                }
            }
            std::vector<uint32_t> ordered;
            PT_HIP(pt_build_order_subset(s->stream, dfs_dev.ptr, d->n_objects, mask, n_selected, ordered));
            dfs.assign(ordered.begin(), ordered.end());
        }
    }
    else {
        // ---- host: leaf boxes, the recursion of pt_bvh.cpp, breadth-first flattening, records -----------------------------------
        std::vector<ptb::Box> boxes(d->n_objects);
        for(uint32_t i = 0; i < d->n_objects; i++) {
            ptb::Box &b = boxes[i];
            const uint32_t idx = leaf_ref[i] & PT_REF_INDEX;
            if((leaf_ref[i] & PT_REF_SPHERE) == 0) {
                const float *p = d->tri_pos + 9 * static_cast<size_t>(idx);
                for(int k = 0; k < 3; k++) { // Triangle::getBoundingVolume, object.cpp:184-186
                    b.lo[k] = fmin_std(fmin_std(p[k], p[3 + k]), p[6 + k]);
                    b.hi[k] = fmax_std(fmax_std(p[k], p[3 + k]), p[6 + k]);
                }
            }
            else {
                const float *sp = d->sph + 4 * static_cast<size_t>(idx);
                for(int k = 0; k < 3; k++) { // Sphere::getBoundingVolume, object.cpp:90-93
                    b.lo[k] = sp[k] - sp[3];
                    b.hi[k] = sp[k] + sp[3];
                }
            }
        }
        int threads = env_int("PT_BUILD_THREADS", static_cast<int>(std::thread::hardware_concurrency()));
        threads = std::max(1, std::min(threads, 64));
        s->tree = ptb::build_reference_bvh(boxes, threads);
        s->depth = s->tree.depth;
        if(s->depth > PT_MAX_DEPTH) {
            return fail(PT_ERR_UNSUPPORTED, "internal: BVH deeper than 128 levels (impl::constructBVH keeps a child at two thirds of its parent at most: 53 levels for 2^30 objects; tests/test_oracle_golden.py)");
        }
        ptb::FlatBvh flat = ptb::flatten_breadth_first(s->tree, leaf_ref, align_siblings);
        n_pairs = flat.n_pairs;
        root_ref = flat.root_ref;
        for(int k = 0; k < 3; k++) {
            root_lo[k] = flat.root_box.lo[k];
            root_hi[k] = flat.root_box.hi[k];
        }
        ptb::leaves_depth_first(s->tree, dfs);
        s->build_ms[0] = ms_since(t_begin);
        const auto t_upload = clock::now();

        std::vector<F4> tris(PT_TRI_QUADS * (static_cast<size_t>(d->n_triangles) + 1 + d->n_spheres), F4{0.0F, 0.0F, 0.0F, 0.0F}), shade(8 * static_cast<size_t>(d->n_triangles), F4{0.0F, 0.0F, 0.0F, 0.0F});
        for(uint32_t t = 0; t < d->n_triangles; t++) {
            const float *p = d->tri_pos + 9 * static_cast<size_t>(t);
            const Vec3 a = ld(p), b = ld(p + 3), c = ld(p + 6);
            const Vec3 ab = sub(b, a), ac = sub(c, a);
            const uint32_t obj_cull = s->tri_obj[t] | (d->tri_cull[t] != 0 ? 0x80000000U : 0U);
            tris[PT_TRI_QUADS * static_cast<size_t>(t) + 0] = {a.x, a.y, a.z, ab.x};
            tris[PT_TRI_QUADS * static_cast<size_t>(t) + 1] = {ab.y, ab.z, ac.x, ac.y};
            tris[PT_TRI_QUADS * static_cast<size_t>(t) + 2] = {ac.z, from_bits(d->tri_material[t]), from_bits(obj_cull), 0.0F};
            Vec3 na, nb, nc;
            if(d->tri_nrm != nullptr) {
                const float *q = d->tri_nrm + 9 * static_cast<size_t>(t);
                na = ld(q);
                nb = ld(q + 3);
                nc = ld(q + 6);
            }
            else {
                na = nb = nc = normalize(cross(ab, ac)); // Triangle::Triangle, object.cpp:118-124
            }
            for(int k = 0; k < 3; k++) {
                shade[8 * static_cast<size_t>(t) + k] = tris[PT_TRI_QUADS * static_cast<size_t>(t) + k];
            }
            shade[8 * static_cast<size_t>(t) + 3] = {na.x, na.y, na.z, nb.x};
            shade[8 * static_cast<size_t>(t) + 4] = {nb.y, nb.z, nc.x, nc.y};
            shade[8 * static_cast<size_t>(t) + 5] = {nc.z, 0.0F, 0.0F, 0.0F};
        }
        std::vector<F4> spheres(d->n_spheres);
        std::vector<uint2> sph_meta(d->n_spheres);
        for(uint32_t i = 0; i < d->n_spheres; i++) {
            const float *sp = d->sph + 4 * static_cast<size_t>(i);
            spheres[i] = {sp[0], sp[1], sp[2], sp[3]};
            tris[PT_TRI_QUADS * (static_cast<size_t>(d->n_triangles) + 1 + i)] = spheres[i]; // the record the traversal fetches (pt_types.h)
            sph_meta[i] = make_uint2(d->sph_material[i], s->sph_obj[i]);
        }
        std::vector<F4> pairs(4 * static_cast<size_t>(flat.n_pairs));
        std::memcpy(pairs.data(), flat.pairs.data(), flat.pairs.size() * sizeof(float));
        PT_HIP(s->pairs.upload(pairs));
        PT_HIP(s->tris.upload(tris));
        PT_HIP(s->tri_shade.upload(shade));
        PT_HIP(s->spheres.upload(spheres));
        PT_HIP(s->sph_meta.upload(sph_meta));
        s->build_ms[1] = ms_since(t_upload);
    }
    const auto t_rest = clock::now();

    std::vector<F4> materials(4 * static_cast<size_t>(d->n_materials));
    for(uint32_t i = 0; i < d->n_materials; i++) {
        const pt_material &m = d->materials[i];
        materials[4 * static_cast<size_t>(i) + 0] = {m.diffuse[0], m.diffuse[1], m.diffuse[2], m.diffuse[3]};
        materials[4 * static_cast<size_t>(i) + 1] = {m.specular[0], m.specular[1], m.specular[2], m.specular[3]};
        materials[4 * static_cast<size_t>(i) + 2] = {m.emission[0], m.emission[1], m.emission[2], m.emission[3]};
        materials[4 * static_cast<size_t>(i) + 3] = {m.ior, from_bits(static_cast<uint32_t>(m.bsdf)), from_bits(static_cast<uint32_t>(m.one_way != 0)), 0.0F};
        if(m.bsdf < PT_BSDF_LAMBERTIAN || m.bsdf > PT_BSDF_MIRROR) {
            return fail(PT_ERR_INVALID, "unknown BSDF kind");
        }
    }
    std::vector<F4> lights(2 * static_cast<size_t>(d->n_point_lights));
    for(uint32_t i = 0; i < d->n_point_lights; i++) {
        const float *p = d->light_pos + 3 * static_cast<size_t>(i);
        const float *c = d->light_spectrum + 4 * static_cast<size_t>(i);
        lights[2 * static_cast<size_t>(i) + 0] = {p[0], p[1], p[2], 0.0F};
        lights[2 * static_cast<size_t>(i) + 1] = {c[0], c[1], c[2], c[3]};
    }

    // ---- emissive objects: Scene::registerEmissiveObjects + CDF (scene.cpp:183-208, 167-180) -----------------------------------
    std::vector<F4> emis;
    std::vector<float> cdf;
    const float pi = static_cast<float>(M_PI);
    for(int32_t obj : dfs) {
        const uint32_t ref = leaf_ref[obj];
        const uint32_t idx = ref & PT_REF_INDEX;
        const bool is_sphere = (ref & PT_REF_SPHERE) != 0;
        const uint32_t mat = is_sphere ? d->sph_material[idx] : d->tri_material[idx];
        if(mat == PT_NO_MATERIAL) {
            continue; // default material has no emission
        }
        const float *e = d->materials[mat].emission;
        const float emissive_power = (e[0] + e[1] + e[2]) * e[3];
        if(emissive_power <= 0.0F) {
            continue;
        }
        float area;
        if(is_sphere) {
            const float r = d->sph[4 * static_cast<size_t>(idx) + 3];
            area = 4.0F * pi * (r * r); // object.cpp:95-99
        }
        else {
            const float *p = d->tri_pos + 9 * static_cast<size_t>(idx);
            const Vec3 c = cross(sub(ld(p + 3), ld(p)), sub(ld(p + 6), ld(p)));
            area = std::sqrt(dot(c, c)) / 2.0F; // object.cpp:188-190
        }
        const float object_probability = emissive_power * area;
        if(object_probability <= 0.0F) {
            continue;
        }
        if(is_sphere) {
            const float *sp = d->sph + 4 * static_cast<size_t>(idx);
            emis.push_back({sp[0], sp[1], sp[2], sp[3]});
            emis.push_back({0.0F, 0.0F, 0.0F, 0.0F});
            emis.push_back({0.0F, from_bits(ref), 0.0F, from_bits(mat)});
        }
        else {
            const float *p = d->tri_pos + 9 * static_cast<size_t>(idx);
            emis.push_back({p[0], p[1], p[2], p[3]});
            emis.push_back({p[4], p[5], p[6], p[7]});
            emis.push_back({p[8], from_bits(ref), from_bits(d->tri_cull[idx] != 0 ? 1U : 0U), from_bits(mat)});
        }
        emis.push_back({e[0], e[1], e[2], e[3]});
        cdf.push_back(object_probability);
        s->emissive_obj.push_back(obj);
    }
    {
        float cumulative_probability = 0.0F;
        for(float &v : cdf) {
            const float probability = v;
            v += cumulative_probability;
            cumulative_probability += probability;
        }
        for(float &v : cdf) {
            v /= cumulative_probability;
        }
    }
    s->n_emissive = static_cast<uint32_t>(cdf.size());
    s->emissive_cdf = cdf;
    const int emissive_object_count = static_cast<int>(cdf.size());
    const int object_sample_count = std::min(2 + static_cast<int>(std::log10(emissive_object_count + 1)), emissive_object_count); // scene.cpp:226
    if(d->n_point_lights + static_cast<uint32_t>(object_sample_count) > PT_MAX_NEE) {
        return fail(PT_ERR_UNSUPPORTED, "more than 32 light samples per path vertex (" + std::to_string(d->n_point_lights) + " point lights + " + std::to_string(object_sample_count) +
                                        " emitter samples): the visibility mask of a path vertex has 32 bits");
    }

    // ---- upload --------------------------------------------------------------------------------------------------------------
    PT_HIP(s->materials.upload(materials));
    PT_HIP(s->lights.upload(lights));
    PT_HIP(s->emis.upload(emis));
    PT_HIP(s->emis_cdf.upload(cdf));

    // ---- link: leaf records and pair records become ONE array, and the tree's references indices into it (pt_types.h) --------------
    // (the pair records start on an even record: two sibling nodes on slots 2k, 2k + 1 share one aligned 128-byte line only then)
    const uint32_t sphere_base = d->n_triangles + 1U, leaf_count = sphere_base + d->n_spheres, pair_base = (leaf_count + 1U) & ~1U;
    if(static_cast<uint64_t>(pair_base) + n_pairs > PT_REF_INDEX) {
        return fail(PT_ERR_UNSUPPORTED, "too many records for 30-bit references");
    }
    PT_HIP(s->recs.ensure(4 * (static_cast<size_t>(pair_base) + n_pairs)));
    PT_HIP(hipMemcpyAsync(s->recs.ptr, s->tris.ptr, 4 * static_cast<size_t>(leaf_count) * sizeof(F4), hipMemcpyDeviceToDevice, s->stream));
    if(pair_base > leaf_count) {
        PT_HIP(hipMemsetAsync(s->recs.ptr + 4 * static_cast<size_t>(leaf_count), 0, 4 * sizeof(F4), s->stream));
    }
    if(n_pairs > 0) {
        PT_HIP(hipMemcpyAsync(s->recs.ptr + 4 * static_cast<size_t>(pair_base), s->pairs.ptr, 4 * static_cast<size_t>(n_pairs) * sizeof(F4), hipMemcpyDeviceToDevice, s->stream));
        PT_HIP(pt_link_records(s->stream, reinterpret_cast<float4 *>(s->recs.ptr), pair_base, n_pairs, sphere_base));
    }
    PT_HIP(hipStreamSynchronize(s->stream));
    s->tris.release();
    s->pairs.release();
    if(root_ref != PT_REF_NONE) {
        root_ref += (root_ref & PT_REF_LEAF) == 0 ? pair_base : ((root_ref & PT_REF_SPHERE) != 0 ? sphere_base : 0U);
    }

    PtDevScene &dev = s->dev;
    dev.recs = reinterpret_cast<const float4 *>(s->recs.ptr);
    dev.pairs = dev.recs + 4 * static_cast<size_t>(pair_base);
    dev.tris = dev.recs;
    dev.pair_base = pair_base;
    dev.tri_shade = reinterpret_cast<const float4 *>(s->tri_shade.ptr);
    dev.spheres = reinterpret_cast<const float4 *>(s->spheres.ptr);
    dev.sph_meta = s->sph_meta.ptr;
    dev.materials = reinterpret_cast<const float4 *>(s->materials.ptr);
    dev.lights = reinterpret_cast<const float4 *>(s->lights.ptr);
    dev.emis = reinterpret_cast<const float4 *>(s->emis.ptr);
    dev.emis_cdf = s->emis_cdf.ptr;
    for(int k = 0; k < 3; k++) {
        dev.root_lo[k] = root_lo[k];
        dev.root_hi[k] = root_hi[k];
    }
    dev.root_ref = root_ref;
    dev.n_pairs = n_pairs;
    dev.n_tris = d->n_triangles;
    dev.n_spheres = d->n_spheres;
    dev.n_lights = d->n_point_lights;
    dev.n_emis = s->n_emissive;
    dev.n_materials = d->n_materials;
    dev.n_object_samples = static_cast<uint32_t>(object_sample_count);
    // LDS staging: a scene whose whole tree and leaf records fit in LDS NEXT TO everything else a workgroup keeps there, four workgroups
    // to the CU, lives in LDS entirely (the path kernel's IN_LDS variant): up to 15.8 KB of records with the small stack window, i.e. about
    // 120 triangles.  Larger ones are read through the caches like any tree: staged at three workgroups per CU they are slower than that
    // (176 triangles: 754 against 785 Msamples/s; at two, 256 triangles: 581 against 715 -- profiles/r03_lds_threshold.txt; round 2 staged up to
    // 24 KB).  An LDS copy of only the top of a larger tree was measured in round 1 and does not pay.  PT_LDS_SMALL_BYTES overrides the limit.
    const size_t small_bytes = (static_cast<size_t>(n_pairs) + pair_base) * 64;
    const int wide_word = d->n_point_lights + static_cast<uint32_t>(object_sample_count) > 8U ? 1 : 0;
    const size_t other_lds = pt_path_lds_bytes(wide_word, std::min(std::max(env_int("PT_ROWS", 4), 1), PT_MAX_ROWS), 4, 0U, 0U);
    const size_t room = other_lds < 40960 ? 40960 - other_lds : 0;
    if(small_bytes <= static_cast<size_t>(std::max(env_int("PT_LDS_SMALL_BYTES", static_cast<int>(room)), 0)) && env_int("PT_LDS_SMALL", 1) != 0) {
        dev.n_lds_pairs = n_pairs;
        dev.n_lds_tris = d->n_triangles;
    }
    else {
        dev.n_lds_pairs = 0;
        dev.n_lds_tris = 0;
    }

    int rc = setup_path(s.get());
    if(rc != PT_OK) {
        return rc;
    }
    s->build_ms[3] = ms_since(t_rest);
    if(env_int("PT_DEBUG", 0) != 0) {
        std::fprintf(stderr, "[pt] scene build (%s): %u objects, %u pair records, depth %u; host preparation %.1f ms, upload %.1f ms, device tree %.1f ms, rest %.1f ms\n",
                     s->device_built ? "device" : "host", d->n_objects, n_pairs, s->depth, s->build_ms[0], s->build_ms[1], s->build_ms[2], s->build_ms[3]);
    }
    *out = s.release();
    return PT_OK;
}

void pt_scene_destroy(pt_scene *scene) {
    if(scene == nullptr) {
        return;
    }
    (void)hipSetDevice(scene->device);
    if(scene->stream != nullptr) {
        (void)hipStreamSynchronize(scene->stream);
    }
    delete scene;
}

int pt_scene_info(const pt_scene *scene, uint64_t *n_nodes, uint32_t *depth, uint32_t *n_emissive) {
    if(scene == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    if(n_nodes != nullptr) {
        *n_nodes = scene->n_nodes;
    }
    if(depth != nullptr) {
        *depth = scene->depth;
    }
    if(n_emissive != nullptr) {
        *n_emissive = scene->n_emissive;
    }
    return PT_OK;
}

int pt_scene_emissive(const pt_scene *scene, int32_t *out_obj, float *out_cdf, uint64_t capacity, uint64_t *n_written) {
    if(scene == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    const uint64_t n = std::min<uint64_t>(scene->emissive_obj.size(), capacity);
    for(uint64_t i = 0; i < n; i++) {
        if(out_obj != nullptr) {
            out_obj[i] = scene->emissive_obj[i];
        }
        if(out_cdf != nullptr) {
            out_cdf[i] = scene->emissive_cdf[i];
        }
    }
    if(n_written != nullptr) {
        *n_written = scene->emissive_obj.size();
    }
    return PT_OK;
}

int pt_scene_bvh_dump(const pt_scene *scene, int32_t *out_obj, float *out_box, uint64_t capacity, uint64_t *n_written) {
    if(scene == nullptr || out_obj == nullptr || out_box == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::vector<int32_t> obj;
    std::vector<ptb::Box> box;
    if(!scene->device_built) {
        ptb::dump_preorder(scene->tree, obj, box);
    }
    else {
        // rebuild the pre-order listing from the pair records in HBM
        const uint32_t pair_base = scene->dev.pair_base, sphere_base = scene->dev.n_tris + 1U;
        std::vector<F4> pairs(4 * static_cast<size_t>(scene->dev.n_pairs));
        if(hipSetDevice(scene->device) != hipSuccess ||
           hipMemcpy(pairs.data(), scene->dev.pairs, pairs.size() * sizeof(F4), hipMemcpyDeviceToHost) != hipSuccess) {
            return fail(PT_ERR_HIP, "downloading the pair records failed");
        }
        struct Item {
            uint32_t ref;
            ptb::Box box;
        };
        ptb::Box root;
        for(int k = 0; k < 3; k++) {
            root.lo[k] = scene->dev.root_lo[k];
            root.hi[k] = scene->dev.root_hi[k];
        }
        std::vector<Item> stack{{scene->dev.root_ref, root}};
        obj.reserve(scene->n_nodes);
        box.reserve(scene->n_nodes);
        while(!stack.empty()) {
            const Item it = stack.back();
            stack.pop_back();
            box.push_back(it.box);
            if((it.ref & PT_REF_LEAF) != 0) {
                const uint32_t idx = it.ref & PT_REF_INDEX; // (record indices: pt_types.h)
                obj.push_back(static_cast<int32_t>((it.ref & PT_REF_SPHERE) != 0 ? scene->sph_obj[idx - sphere_base] : scene->tri_obj[idx]));
            }
            else {
                obj.push_back(-1);
                const float *q = &pairs[4 * static_cast<size_t>(it.ref - pair_base)].x;
                Item l, r;
                std::memcpy(&l.box, q, 24);
                std::memcpy(&r.box, q + 6, 24);
                std::memcpy(&l.ref, q + 12, 4);
                std::memcpy(&r.ref, q + 13, 4);
                stack.push_back(r);
                stack.push_back(l);
            }
        }
    }
    const uint64_t n = std::min<uint64_t>(obj.size(), capacity);
    for(uint64_t i = 0; i < n; i++) {
        out_obj[i] = obj[i];
        std::memcpy(out_box + 6 * i, &box[i], sizeof(float) * 6);
    }
    if(n_written != nullptr) {
        *n_written = obj.size();
    }
    return PT_OK;
}

int pt_intersect_batch(pt_scene *s, const float *rays, size_t n, float *out_t, int32_t *out_obj) {
    if(s == nullptr || (n > 0 && (rays == nullptr || out_t == nullptr || out_obj == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(n == 0) {
        return PT_OK;
    }
    if(n > 0x7fffffffULL) {
        return fail(PT_ERR_INVALID, "too many rays in one batch");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    const uint32_t n32 = static_cast<uint32_t>(n);
    {
        int rc = setup_path(s);
        if(rc != PT_OK) {
            return rc;
        }
        PtPathConfig cfg = s->path_cfg;
        PT_HIP(s->batch_rays.ensure(6 * n));
        PT_HIP(s->closest_out.ensure(n));
        PT_HIP(s->path_spill.ensure(((n + 255) / 256) * 256 * cfg.spill_depth));
        cfg.spill = s->path_spill.ptr;
        hipStream_t st = s->stream;
        PT_HIP(hipMemcpyAsync(s->batch_rays.ptr, rays, 6 * n * sizeof(float), hipMemcpyHostToDevice, st));
        pt_launch_closest(st, s->dev, s->batch_rays.ptr, n32, s->closest_out.ptr, cfg);
        PT_HIP(hipGetLastError());
        std::vector<uint2> hits(n);
        PT_HIP(hipMemcpyAsync(hits.data(), s->closest_out.ptr, n * sizeof(uint2), hipMemcpyDeviceToHost, st));
        PT_HIP(hipStreamSynchronize(st));
        for(size_t i = 0; i < n; i++) {
            const float t = from_bits(hits[i].x);
            const uint32_t ref = hits[i].y;
            out_t[i] = t;
            out_obj[i] = (t < 0.0F || ref == PT_REF_NONE) ? -1 : static_cast<int32_t>((ref & PT_REF_SPHERE) ? s->sph_obj[(ref & PT_REF_INDEX) - (s->dev.n_tris + 1U)] : s->tri_obj[ref & PT_REF_INDEX]);
        }
        return PT_OK;
    }
}

// Diagnostic, not part of include/pt_hip.h: walks n rays, `lanes_per_wave` of them per wavefront, with every traversal step stamped.
// out[4 * i ..] = steps, cycles spent waiting for records (flags bit 1: stamped run), cycles of the whole walk, -; flags bit 0: unused;
// behind the n results, 8 segment totals of 8 bytes per ray from a -DPT_STEP_STAMPS build (zeros otherwise): out holds 20 * n words (tools/step_timing.py).
// Diagnostics of the cost-aware placement (tools/place_probe.py): record what every stream of the following launches costs / read the
// last launch's costs / give the NEXT launch its first round as a table (waves x slots_per_wave entries, 0xffffffff = empty slot).
extern "C" int pt_debug_collect_costs(pt_scene *s, int on) {
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    s->debug_collect_costs = on != 0;
    return PT_OK;
}

extern "C" int pt_debug_stream_costs(pt_scene *s, uint32_t *out, size_t n) {
    if(s == nullptr || out == nullptr || n > s->stream_cost.count) {
        return fail(PT_ERR_INVALID, "no costs of that many streams");
    }
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(hipStreamSynchronize(s->stream));
    PT_HIP(hipMemcpy(out, s->stream_cost.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_debug_set_place(pt_scene *s, uint32_t waves, uint32_t slots_per_wave, const uint32_t *table) {
    if(s == nullptr || table == nullptr || waves == 0 || waves % 4U != 0 || slots_per_wave == 0) {
        return fail(PT_ERR_INVALID, "placement table");
    }
    s->debug_place.assign(table, table + static_cast<size_t>(waves) * slots_per_wave);
    s->debug_place_waves = waves;
    s->debug_place_slots = slots_per_wave;
    return PT_OK;
}

extern "C" int pt_debug_step_timing(pt_scene *s, const float *rays, size_t n, int lanes_per_wave, int flags, uint32_t *out) {
    if(s == nullptr || rays == nullptr || out == nullptr || n == 0 || n > 0x3fffffULL || lanes_per_wave < 1 || lanes_per_wave > 64) {
        return fail(PT_ERR_INVALID, "bad argument");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    int rc = setup_path(s);
    if(rc != PT_OK) {
        return rc;
    }
    if(s->path_cfg.in_lds) {
        return fail(PT_ERR_UNSUPPORTED, "step timing is for scenes in HBM");
    }
    const size_t waves = (n + static_cast<size_t>(lanes_per_wave) - 1) / static_cast<size_t>(lanes_per_wave);
    const size_t threads = (waves + 3) / 4 * 256;
    DevBuf<float> d_rays;
    DevBuf<uint4> d_out;
    DevBuf<uint2> d_spill;
    PT_HIP(d_rays.ensure(6 * n));
    PT_HIP(d_out.ensure(5 * n));
    PT_HIP(hipMemsetAsync(d_out.ptr, 0, 5 * n * sizeof(uint4), s->stream));
    PT_HIP(d_spill.ensure(threads * s->path_cfg.spill_depth));
    hipStream_t st = s->stream;
    PT_HIP(hipMemcpyAsync(d_rays.ptr, rays, 6 * n * sizeof(float), hipMemcpyHostToDevice, st));
    pt_launch_steptime(st, s->dev, d_rays.ptr, static_cast<uint32_t>(n), static_cast<uint32_t>(lanes_per_wave), d_out.ptr, d_spill.ptr, s->path_cfg.spill_depth, flags);
    PT_HIP(hipGetLastError());
    PT_HIP(hipMemcpyAsync(out, d_out.ptr, 5 * n * sizeof(uint4), hipMemcpyDeviceToHost, st));
    PT_HIP(hipStreamSynchronize(st));
    return PT_OK;
}

// Diagnostic, not part of include/pt_hip.h: replays the rays the last render left in its rings (PT_RING_LOG_RAYS) through the traversal
// alone, at `waves_per_simd` wavefronts per SIMD with every ring cut into `parts`.  out[0..4] = rays, node visits, leaf tests, wave
// steps, checksum; *out_ms = kernel time; *out_blocks = resident workgroups per CU.
extern "C" int pt_debug_replay_rays(pt_scene *s, int waves_per_simd, int parts, unsigned long long *out, float *out_ms, int *out_blocks) {
    if(s == nullptr || out == nullptr || out_ms == nullptr || out_blocks == nullptr || parts < 1 || s->path_waves == 0) {
        return fail(PT_ERR_INVALID, "nothing to replay");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg = s->path_cfg;
    const uint32_t waves = s->path_waves * static_cast<uint32_t>(parts);
    PT_HIP(s->path_spill.ensure(static_cast<size_t>(waves) * 64U * cfg.spill_depth));
    PT_HIP(s->path_wave_counters.ensure(8));
    PT_HIP(hipMemsetAsync(s->path_wave_counters.ptr, 0, 8 * sizeof(unsigned long long), s->stream));
    PtLocalQueue Q{};
    Q.ray_o = reinterpret_cast<float4 *>(s->lq_ray_o.ptr);
    Q.ray_d = reinterpret_cast<float4 *>(s->lq_ray_d.ptr);
    Q.cap = s->path_cap;
    Event e0, e1;
    PT_HIP(e0.create());
    PT_HIP(e1.create());
    PT_HIP(hipEventRecord(e0.e, s->stream));
    *out_blocks = pt_launch_replay(s->stream, s->dev, Q, s->path_waves, static_cast<uint32_t>(parts), waves_per_simd, cfg, s->path_spill.ptr, s->path_wave_counters.ptr);
    PT_HIP(hipGetLastError());
    PT_HIP(hipEventRecord(e1.e, s->stream));
    PT_HIP(hipMemcpyAsync(out, s->path_wave_counters.ptr, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    PT_HIP(hipEventElapsedTime(out_ms, e0.e, e1.e));
    return PT_OK;
}


int pt_render_streams(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_stream *streams, size_t n, float *out_image,
                      uint64_t *out_states, pt_stats *stats) {
    int rc = check_render_args(s, camera, options);
    if(rc != PT_OK) {
        return rc;
    }
    if(n > 0 && (streams == nullptr || out_image == nullptr)) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(stats != nullptr) {
        std::memset(stats, 0, sizeof(*stats));
    }
    if(n == 0) {
        return PT_OK;
    }
    if(n > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "too many streams");
    }
    PtDevOptions opt;
    rc = derive_options(options, &opt);
    if(rc != PT_OK) {
        return rc;
    }
    const PtDevCamera cam = derive_camera(camera);
    std::vector<int4> rects(n);
    std::vector<uint64_t> states(n);
    for(size_t i = 0; i < n; i++) {
        const pt_stream &t = streams[i];
        if(t.w < 0 || t.h < 0 || t.x < 0 || t.y < 0 || t.x + t.w > options->image_width || t.y + t.h > options->image_height) {
            return fail(PT_ERR_INVALID, "stream rectangle outside the image");
        }
        rects[i] = make_int4(t.x, t.y, t.w, t.h);
        states[i] = t.rng_state;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    const uint32_t n32 = static_cast<uint32_t>(n);
    const size_t pixels = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    PT_HIP(s->image.ensure(pixels));
    hipStream_t st = s->stream;
    {
        PT_HIP(s->st_rect.ensure(n));
        PT_HIP(s->st_rng.ensure(n));
        // pixels not covered by a stream keep the caller's values
        PT_HIP(hipMemcpyAsync(s->image.ptr, out_image, pixels * sizeof(F4), hipMemcpyHostToDevice, st));
        PT_HIP(hipMemcpyAsync(s->st_rect.ptr, rects.data(), n * sizeof(int4), hipMemcpyHostToDevice, st));
        PT_HIP(hipMemcpyAsync(s->st_rng.ptr, states.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        PtStreams T{};
        T.n = n32;
        T.rect = s->st_rect.ptr;
        T.rng = s->st_rng.ptr;
        rc = run_path(s, cam, opt, T, reinterpret_cast<float4 *>(s->image.ptr), stats, nullptr, nullptr);
        if(rc != PT_OK) {
            (void)hipStreamSynchronize(st); // rects / states are this function's vectors
            return rc;
        }
        PT_HIP(hipMemcpyAsync(out_image, s->image.ptr, pixels * sizeof(F4), hipMemcpyDeviceToHost, st));
        if(out_states != nullptr) {
            PT_HIP(hipMemcpyAsync(out_states, s->st_rng.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        }
        return finish_path(s);
    }
}

// A regular grid of equal tiles (what pt_job_tiles makes of a frame whose sides are multiples of the tile size) lets the kernel spread a
// wavefront's first rows over the frame's columns as well as over its bands: tiles per grid row, 64-stream chunks per tile (0, 0: no grid).
static void tile_grid(const pt_tile *tiles, size_t n_tiles, uint32_t *tiles_per_row, uint32_t *chunks_per_tile) {
    *tiles_per_row = 0;
    *chunks_per_tile = 0;
    if(n_tiles > 0 && (static_cast<uint32_t>(tiles[0].w) * static_cast<uint32_t>(tiles[0].h)) % 64U == 0) {
        bool regular = true;
        uint32_t per_row = 0;
        for(size_t k = 0; k < n_tiles && regular; k++) {
            regular = tiles[k].w == tiles[0].w && tiles[k].h == tiles[0].h;
            if(per_row == 0 && k > 0 && tiles[k].y != tiles[0].y) {
                per_row = static_cast<uint32_t>(k);
            }
        }
        if(per_row == 0) {
            per_row = static_cast<uint32_t>(n_tiles);
        }
        for(size_t k = 0; k < n_tiles && regular; k++) {
            regular = tiles[k].x == tiles[0].x + static_cast<int32_t>(k % per_row) * tiles[0].w && tiles[k].y == tiles[0].y + static_cast<int32_t>(k / per_row) * tiles[0].h;
        }
        if(regular && n_tiles % per_row == 0 && per_row % 4 == 0) {
            *tiles_per_row = per_row;
            *chunks_per_tile = static_cast<uint32_t>(tiles[0].w) * static_cast<uint32_t>(tiles[0].h) / 64U;
        }
    }
}

// A view batch (pt_render_views): n > 1 views of one scene whose frames are stacked into one image of n * image_height rows; view v has the
// camera cams[v] and the seed seeds[v].  The tiles of such a call lie in the stacked image.
struct ViewSet {
    std::vector<PtViewCamera> cams;
    std::vector<uint64_t> seeds;
    int32_t rows(const pt_options *options) const { return static_cast<int32_t>(cams.size()) * options->image_height; }
};

static int render_tiles_impl(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles, uint64_t base_seed,
                             float4 *d_image, pt_stats *stats, pt_progress_fn progress = nullptr, void *progress_user = nullptr, RenderStop *stop = nullptr,
                             const ViewSet *views = nullptr) {
    PtDevOptions opt;
    int rc = derive_options(options, &opt);
    if(rc != PT_OK) {
        return rc;
    }
    const PtDevCamera cam = derive_camera(camera);
    const int32_t rows = views != nullptr ? views->rows(options) : options->image_height;
    uint64_t total = 0;
    for(size_t i = 0; i < n_tiles; i++) {
        const pt_tile &t = tiles[i];
        if(t.w <= 0 || t.h <= 0 || t.x < 0 || t.y < 0 || t.x + t.w > options->image_width || t.y + t.h > rows) {
            return fail(PT_ERR_INVALID, "tile outside the image or empty");
        }
        total += static_cast<uint64_t>(t.w) * static_cast<uint64_t>(t.h);
    }
    if(total > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "too many pixels in one call");
    }
    const uint32_t n32 = static_cast<uint32_t>(total);
    {
        // stream i = pixel i of the tiles laid end to end; the kernel derives rectangle and engine from the tile table
        std::vector<int4> rects(n_tiles);
        std::vector<uint32_t> offsets(n_tiles), left(n_tiles);
        uint64_t at = 0;
        for(size_t k = 0; k < n_tiles; k++) {
            const pt_tile &t = tiles[k];
            rects[k] = make_int4(t.x, t.y, t.w, t.h);
            offsets[k] = static_cast<uint32_t>(at);
            left[k] = static_cast<uint32_t>(t.w) * static_cast<uint32_t>(t.h);
            at += left[k];
        }
        PT_HIP(s->tiles.ensure(n_tiles));
        PT_HIP(s->tile_offset.ensure(n_tiles));
        hipStream_t st = s->stream;
        PT_HIP(hipMemcpyAsync(s->tiles.ptr, rects.data(), n_tiles * sizeof(int4), hipMemcpyHostToDevice, st));
        PT_HIP(hipMemcpyAsync(s->tile_offset.ptr, offsets.data(), n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if(progress != nullptr || stop != nullptr) {
            PT_HIP(s->tile_left.ensure(n_tiles));
            PT_HIP(hipMemcpyAsync(s->tile_left.ptr, left.data(), n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        if(views != nullptr) {
            PT_HIP(s->view_cams.ensure(views->cams.size()));
            PT_HIP(s->view_seeds.ensure(views->seeds.size()));
            PT_HIP(hipMemcpyAsync(s->view_cams.ptr, views->cams.data(), views->cams.size() * sizeof(PtViewCamera), hipMemcpyHostToDevice, st));
            PT_HIP(hipMemcpyAsync(s->view_seeds.ptr, views->seeds.data(), views->seeds.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        }
        PT_HIP(hipStreamSynchronize(st)); // the tables are this function's vectors
        PtStreams T{};
        T.n = n32;
        T.tiles = s->tiles.ptr;
        T.tile_offset = s->tile_offset.ptr;
        T.n_tiles = static_cast<uint32_t>(n_tiles);
        T.base_seed = base_seed;
        if(views != nullptr) {
            T.n_views = static_cast<uint32_t>(views->cams.size());
            T.view_height = static_cast<uint32_t>(options->image_height);
            T.views = s->view_cams.ptr;
            T.view_seed = s->view_seeds.ptr;
        }
        // A regular grid of equal tiles (what pt_job_tiles makes of a frame whose sides are multiples of the tile size) lets the kernel
        // spread a wavefront's first rows over the frame's columns as well as over its bands: tiles per grid row, 64-stream chunks per tile.
        tile_grid(tiles, n_tiles, &T.tiles_per_row, &T.chunks_per_tile);
        return run_path(s, cam, opt, T, d_image, stats, progress, progress_user, nullptr, false, stop);
    }
}

int pt_render_tiles(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles, uint64_t base_seed,
                    float *out_image, pt_stats *stats) {
    return pt_render_tiles_progress(s, camera, options, tiles, n_tiles, base_seed, out_image, stats, nullptr, nullptr);
}

int pt_render_tiles_progress(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles, uint64_t base_seed,
                             float *out_image, pt_stats *stats, pt_progress_fn progress, void *progress_user) {
    int rc = check_render_args(s, camera, options);
    if(rc != PT_OK) {
        return rc;
    }
    if(stats != nullptr) {
        std::memset(stats, 0, sizeof(*stats));
    }
    if(n_tiles == 0) {
        return PT_OK;
    }
    if(tiles == nullptr || out_image == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    const size_t pixels = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    PT_HIP(s->image.ensure(pixels));
    PT_HIP(hipMemcpyAsync(s->image.ptr, out_image, pixels * sizeof(F4), hipMemcpyHostToDevice, s->stream));
    rc = render_tiles_impl(s, camera, options, tiles, n_tiles, base_seed, reinterpret_cast<float4 *>(s->image.ptr), stats, progress, progress_user);
    if(rc != PT_OK) {
        return rc;
    }
    PT_HIP(hipMemcpyAsync(out_image, s->image.ptr, pixels * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
    return finish_path(s);
}

int pt_render_item(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_stream *item, float *out_tile, uint64_t *out_state,
                   pt_stats *stats) {
    int rc = check_render_args(s, camera, options);
    if(rc != PT_OK) {
        return rc;
    }
    if(item == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(stats != nullptr) {
        std::memset(stats, 0, sizeof(*stats));
    }
    if(item->w < 0 || item->h < 0 || item->x < 0 || item->y < 0 || item->x + item->w > options->image_width || item->y + item->h > options->image_height) {
        return fail(PT_ERR_INVALID, "work item outside the image");
    }
    if(out_state != nullptr) {
        *out_state = item->rng_state;
    }
    if(item->w == 0 || item->h == 0) {
        return PT_OK; // a zero-area WorkItem renders nothing and leaves its engine untouched
    }
    if(out_tile == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    PtDevOptions opt;
    rc = derive_options(options, &opt);
    if(rc != PT_OK) {
        return rc;
    }
    const PtDevCamera cam = derive_camera(camera);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    // the frame exists in device memory only; the host sees the item's rectangle
    const size_t pixels = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    PT_HIP(s->image.ensure(pixels));
    PT_HIP(s->st_rect.ensure(1));
    PT_HIP(s->st_rng.ensure(1));
    hipStream_t st = s->stream;
    const int4 rect = make_int4(item->x, item->y, item->w, item->h);
    PT_HIP(hipMemcpyAsync(s->st_rect.ptr, &rect, sizeof(rect), hipMemcpyHostToDevice, st));
    PT_HIP(hipMemcpyAsync(s->st_rng.ptr, &item->rng_state, sizeof(uint64_t), hipMemcpyHostToDevice, st));
    PT_HIP(hipStreamSynchronize(st));
    PtStreams T{};
    T.n = 1;
    T.rect = s->st_rect.ptr;
    T.rng = s->st_rng.ptr;
    rc = run_path(s, cam, opt, T, reinterpret_cast<float4 *>(s->image.ptr), stats, nullptr, nullptr);
    if(rc != PT_OK) {
        return rc;
    }
    const F4 *first = s->image.ptr + static_cast<size_t>(item->y) * static_cast<size_t>(options->image_width) + static_cast<size_t>(item->x);
    PT_HIP(hipMemcpy2DAsync(out_tile, static_cast<size_t>(item->w) * sizeof(F4), first, static_cast<size_t>(options->image_width) * sizeof(F4),
                            static_cast<size_t>(item->w) * sizeof(F4), static_cast<size_t>(item->h), hipMemcpyDeviceToHost, st));
    if(out_state != nullptr) {
        PT_HIP(hipMemcpyAsync(out_state, s->st_rng.ptr, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    return finish_path(s);
}

} // extern "C"

// The replica that renders each tile of a multi-device call (render_tiles_multi_impl, and a frame's tiles for good: pt_frame_create).
static std::vector<int> tile_owners(const pt_tile *tiles, size_t n_tiles, int n_scenes) {
    size_t per_row = 0;
    while(per_row < n_tiles && tiles[per_row].y == tiles[0].y) {
        per_row++;
    }
    const bool diagonal = n_scenes > 1 && per_row > 0 && n_tiles % per_row == 0 && per_row % static_cast<size_t>(n_scenes) == 0;
    std::vector<int> owners(n_tiles);
    for(size_t k = 0; k < n_tiles; k++) {
        owners[k] = static_cast<int>((diagonal ? k % per_row + k / per_row : k) % static_cast<size_t>(n_scenes));
    }
    return owners;
}

// pt_render_tiles_multi, and with a RenderStop pt_render_tiles_ctl: then every replica also loads the rectangles of its tiles from out_image
// first (so that the pixels a stopped launch leaves unwritten keep their values), and reports which of its tiles finished and what became of
// its streams (tile_done: [n_tiles] or null, tallies: [n_scenes]).
static int render_tiles_multi_impl(pt_scene *const *scenes, int n_scenes, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles,
                                   uint64_t base_seed, float *out_image, pt_stats *stats, pt_progress_fn progress, void *progress_user, RenderStop *stop = nullptr,
                                   uint8_t *tile_done = nullptr, StreamTally *tallies = nullptr, const ViewSet *views = nullptr) {
    if(scenes == nullptr || n_scenes < 1) {
        return fail(PT_ERR_INVALID, "no scenes");
    }
    for(int i = 0; i < n_scenes; i++) {
        const int rc = check_render_args(scenes[i], camera, options);
        if(rc != PT_OK) {
            return rc;
        }
    }
    if(n_tiles == 0) {
        return PT_OK;
    }
    if(tiles == nullptr || out_image == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    const int32_t rows = views != nullptr ? views->rows(options) : options->image_height; // (a view batch: the stacked image)
    for(size_t k = 0; k < n_tiles; k++) {
        const pt_tile &t = tiles[k];
        if(t.w <= 0 || t.h <= 0 || t.x < 0 || t.y < 0 || t.x + t.w > options->image_width || t.y + t.h > rows) {
            return fail(PT_ERR_INVALID, "tile outside the image or empty");
        }
    }
    // The multi-device form of doWorkParallel (src/worker.cpp:364-387): the tiles are dealt round-robin to the scenes (each a replica on its
    // own device; along the diagonals of a grid whose rows hold a multiple of n_scenes tiles, so that no device gets whole columns of the
    // frame -- cpupathtrace_amd/sharding.py uses the same rule), one host thread per scene drives its device, every device renders into its
    // own frame in HBM and only the rectangles of ITS tiles travel to the caller's image.  Engines are per pixel, so the image does not
    // depend on n_scenes.  progress calls are serialised and counted over all devices.
    const std::vector<int> owners = tile_owners(tiles, n_tiles, n_scenes);
    auto owner = [&](size_t k) -> int {
        return owners[k];
    };
    struct Shared {
        std::mutex progress_mutex;
        int completed = 0, total = 0;
        pt_progress_fn fn = nullptr;
        void *user = nullptr;
    } shared;
    shared.total = static_cast<int>(n_tiles);
    shared.fn = progress;
    shared.user = progress_user;
    auto trampoline = [](int, int, void *p) {
        Shared *sh = static_cast<Shared *>(p);
        std::lock_guard<std::mutex> lock(sh->progress_mutex);
        sh->completed++;
        sh->fn(sh->completed, sh->total, sh->user);
    };
    std::vector<int> rcs(static_cast<size_t>(n_scenes), PT_OK);
    std::vector<std::string> errors(static_cast<size_t>(n_scenes));
    const size_t width = static_cast<size_t>(options->image_width), pixels = width * static_cast<size_t>(rows);
    auto work = [&](int i) {
        std::vector<pt_tile> mine;
        std::vector<size_t> mine_index;
        for(size_t k = 0; k < n_tiles; k++) {
            if(owner(k) == i) {
                mine.push_back(tiles[k]);
                mine_index.push_back(k);
            }
        }
        if(mine.empty()) {
            return;
        }
        pt_scene *s = scenes[i];
        auto run = [&]() -> int {
            std::lock_guard<std::mutex> lock(s->render_mutex);
            PT_HIP(hipSetDevice(s->device));
            PT_HIP(s->image.ensure(pixels));
            if(stop != nullptr) {
                for(const pt_tile &t : mine) {
                    const size_t at = static_cast<size_t>(t.y) * width + static_cast<size_t>(t.x);
                    PT_HIP(hipMemcpy2DAsync(s->image.ptr + at, width * sizeof(F4), out_image + at * 4, width * sizeof(F4), static_cast<size_t>(t.w) * sizeof(F4),
                                            static_cast<size_t>(t.h), hipMemcpyHostToDevice, s->stream));
                }
            }
            int rc = render_tiles_impl(s, camera, options, mine.data(), mine.size(), base_seed, reinterpret_cast<float4 *>(s->image.ptr),
                                       stats != nullptr ? stats + i : nullptr, progress != nullptr ? static_cast<pt_progress_fn>(trampoline) : nullptr, &shared, stop, views);
            if(rc != PT_OK) {
                return rc;
            }
            for(const pt_tile &t : mine) {
                const size_t at = static_cast<size_t>(t.y) * width + static_cast<size_t>(t.x);
                PT_HIP(hipMemcpy2DAsync(out_image + at * 4, width * sizeof(F4), s->image.ptr + at, width * sizeof(F4), static_cast<size_t>(t.w) * sizeof(F4),
                                        static_cast<size_t>(t.h), hipMemcpyDeviceToHost, s->stream));
            }
            if(stop == nullptr) {
                return finish_path(s);
            }
            rc = finish_path(s, &tallies[i]);
            if(rc != PT_OK) {
                return rc;
            }
            if(tile_done != nullptr) {
                // pixels of each tile not finished (render_tiles_impl set them to the tile's size, the kernel counted them down)
                std::vector<uint32_t> left(mine.size());
                PT_HIP(hipMemcpy(left.data(), s->tile_left.ptr, left.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
                for(size_t k = 0; k < mine.size(); k++) {
                    tile_done[mine_index[k]] = left[k] == 0 ? 1 : 0;
                }
            }
            return PT_OK;
        };
        rcs[static_cast<size_t>(i)] = run();
        if(rcs[static_cast<size_t>(i)] != PT_OK) {
            errors[static_cast<size_t>(i)] = g_last_error; // this thread's message
        }
    };
    if(stats != nullptr) {
        std::memset(stats, 0, sizeof(*stats) * static_cast<size_t>(n_scenes));
    }
    std::vector<std::thread> threads;
    for(int i = 1; i < n_scenes; i++) {
        threads.emplace_back(work, i);
    }
    work(0);
    for(std::thread &t : threads) {
        t.join();
    }
    for(int i = 0; i < n_scenes; i++) {
        if(rcs[static_cast<size_t>(i)] != PT_OK) {
            return fail(rcs[static_cast<size_t>(i)], "scene " + std::to_string(i) + ": " + errors[static_cast<size_t>(i)]);
        }
    }
    return PT_OK;
}

extern "C" {

int pt_render_tiles_multi(pt_scene *const *scenes, int n_scenes, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles,
                          uint64_t base_seed, float *out_image, pt_stats *stats, pt_progress_fn progress, void *progress_user) {
    return render_tiles_multi_impl(scenes, n_scenes, camera, options, tiles, n_tiles, base_seed, out_image, stats, progress, progress_user);
}

int pt_render_tiles_ctl(pt_scene *const *scenes, int n_scenes, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles,
                        uint64_t base_seed, float *out_image, pt_stats *stats, pt_progress_fn progress, void *progress_user, pt_render_control *ctl) {
    const RenderStop::Clock::time_point start = RenderStop::Clock::now();
    if(ctl == nullptr) {
        return fail(PT_ERR_INVALID, "null control");
    }
    ctl->streams_finished = ctl->streams_abandoned = ctl->streams_unclaimed = 0;
    ctl->drain_ms = 0.0;
    if(ctl->tile_done != nullptr && n_tiles > 0) {
        std::memset(ctl->tile_done, 0, n_tiles);
    }
    RenderStop stop;
    stop.ctl = ctl;
    if(ctl->budget_ms > 0.0) {
        stop.has_deadline = true;
        stop.deadline = start + std::chrono::duration_cast<RenderStop::Clock::duration>(std::chrono::duration<double, std::milli>(ctl->budget_ms));
    }
    stop.poll(); // (a control cancelled before the call, or a budget spent already: the launches start stopped)
    std::vector<StreamTally> tallies(n_scenes > 0 ? static_cast<size_t>(n_scenes) : 0U);
    const int rc = render_tiles_multi_impl(scenes, n_scenes, camera, options, tiles, n_tiles, base_seed, out_image, stats, progress, progress_user, &stop, ctl->tile_done,
                                           tallies.data());
    if(rc != PT_OK) {
        return rc;
    }
    for(const StreamTally &t : tallies) {
        ctl->streams_finished += t.finished;
        ctl->streams_abandoned += t.abandoned;
        ctl->streams_unclaimed += t.unclaimed;
    }
    ctl->drain_ms = stop.drain_ms;
    if(ctl->streams_abandoned + ctl->streams_unclaimed != 0) {
        return fail(PT_ERR_CANCELLED, "render stopped (" + std::string(__atomic_load_n(&ctl->cancel, __ATOMIC_ACQUIRE) != 0 ? "cancelled" : "budget spent") + "): " +
                                          std::to_string(ctl->streams_abandoned) + " streams abandoned, " + std::to_string(ctl->streams_unclaimed) + " never taken");
    }
    return PT_OK;
}

int pt_render_cancel(pt_render_control *ctl) {
    if(ctl == nullptr) {
        return fail(PT_ERR_INVALID, "null control");
    }
    __atomic_store_n(&ctl->cancel, 1, __ATOMIC_RELEASE);
    return PT_OK;
}

int pt_render_tiles_device(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles, uint64_t base_seed,
                           float *d_out_image, void *stream, pt_stats *stats) {
    int rc = check_render_args(s, camera, options);
    if(rc != PT_OK) {
        return rc;
    }
    if(stats != nullptr) {
        std::memset(stats, 0, sizeof(*stats));
    }
    if(n_tiles == 0) {
        return PT_OK;
    }
    if(tiles == nullptr || d_out_image == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    // order after the caller's stream, render on the library's stream, then make the caller's stream wait for it
    hipStream_t caller = static_cast<hipStream_t>(stream);
    Event ev;
    PT_HIP(ev.create(hipEventDisableTiming));
    PT_HIP(hipEventRecord(ev.e, caller));
    PT_HIP(hipStreamWaitEvent(s->stream, ev.e, 0));
    rc = render_tiles_impl(s, camera, options, tiles, n_tiles, base_seed, reinterpret_cast<float4 *>(d_out_image), stats);
    if(rc == PT_OK) {
        PT_HIP(hipEventRecord(ev.e, s->stream));
        PT_HIP(hipStreamWaitEvent(caller, ev.e, 0));
        // This entry point does not wait for the device (the frame stays in HBM for the caller's stream).  With statistics it has waited
        // and checked already (run_path); PT_VERIFY=1 makes every call wait and check.
        if(stats == nullptr && env_int("PT_VERIFY", 0) != 0) {
            rc = finish_path(s);
        }
    }
    return rc;
}

} // extern "C"

// ---- view batches (pt_render_views*): V cameras of one scene in one launch per replica ------------------------------------------------
// The views' frames are stacked into one image of V * H rows, view v = rows [v H, (v + 1) H), and the job is the tile list pt_job_tiles(W, H)
// of every view, moved down by v H, view after view.  The kernel finds a pixel's view from its row (pt_path.hip): its seed and camera ray
// are what pt_render_tiles(cameras[v], base_seeds[v]) gives the pixel at the local row, and the image store needs no change -- row-major
// W x (V H) is [V][H][W].  One view is that call itself.

// The arguments every view-batch entry point checks before anything is launched; fills the stacked tile list and, for V > 1, the view set.
static int prepare_views(const pt_camera_params *cameras, const uint64_t *base_seeds, int32_t n_views, const pt_options *options, std::vector<pt_tile> *tiles,
                         ViewSet *views) {
    if(cameras == nullptr || base_seeds == nullptr || options == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(n_views <= 0) {
        return fail(PT_ERR_INVALID, "a view batch needs at least one view");
    }
    if(options->image_width <= 0 || options->image_height <= 0) {
        return fail(PT_ERR_INVALID, "image size must be positive");
    }
    const uint64_t rows = static_cast<uint64_t>(n_views) * static_cast<uint64_t>(options->image_height);
    if(rows > 0x7fffffffULL || rows * static_cast<uint64_t>(options->image_width) > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "too many pixels in one call");
    }
    const size_t per_view = pt_job_tiles(options->image_width, options->image_height, nullptr, 0);
    tiles->resize(per_view * static_cast<size_t>(n_views));
    pt_job_tiles(options->image_width, options->image_height, tiles->data(), per_view);
    for(int32_t v = 1; v < n_views; v++) {
        for(size_t k = 0; k < per_view; k++) {
            pt_tile t = (*tiles)[k];
            t.y += v * options->image_height;
            (*tiles)[static_cast<size_t>(v) * per_view + k] = t;
        }
    }
    views->cams.clear();
    views->seeds.clear();
    if(n_views > 1) {
        views->cams.resize(static_cast<size_t>(n_views));
        for(int32_t v = 0; v < n_views; v++) {
            views->cams[static_cast<size_t>(v)] = PtViewCamera{derive_camera(cameras + v), {0, 0, 0}};
        }
        views->seeds.assign(base_seeds, base_seeds + n_views);
    }
    return PT_OK;
}

extern "C" {

int pt_render_views(pt_scene *const *scenes, int n_scenes, const pt_camera_params *cameras, const uint64_t *base_seeds, int32_t n_views, const pt_options *options,
                    float *out_images, pt_stats *stats, pt_progress_fn progress, void *progress_user) {
    std::vector<pt_tile> tiles;
    ViewSet views;
    int rc = prepare_views(cameras, base_seeds, n_views, options, &tiles, &views);
    if(rc != PT_OK) {
        return rc;
    }
    if(out_images == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    return render_tiles_multi_impl(scenes, n_scenes, cameras, options, tiles.data(), tiles.size(), base_seeds[0], out_images, stats, progress, progress_user, nullptr,
                                   nullptr, nullptr, n_views > 1 ? &views : nullptr);
}

int pt_render_views_device(pt_scene *s, const pt_camera_params *cameras, const uint64_t *base_seeds, int32_t n_views, const pt_options *options, float *d_out_images,
                           void *stream, pt_stats *stats) {
    std::vector<pt_tile> tiles;
    ViewSet views;
    int rc = prepare_views(cameras, base_seeds, n_views, options, &tiles, &views);
    if(rc != PT_OK) {
        return rc;
    }
    rc = check_render_args(s, cameras, options);
    if(rc != PT_OK) {
        return rc;
    }
    if(stats != nullptr) {
        std::memset(stats, 0, sizeof(*stats));
    }
    if(d_out_images == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    // ordered after the caller's stream and before its later work, as pt_render_tiles_device
    hipStream_t caller = static_cast<hipStream_t>(stream);
    Event ev;
    PT_HIP(ev.create(hipEventDisableTiming));
    PT_HIP(hipEventRecord(ev.e, caller));
    PT_HIP(hipStreamWaitEvent(s->stream, ev.e, 0));
    rc = render_tiles_impl(s, cameras, options, tiles.data(), tiles.size(), base_seeds[0], reinterpret_cast<float4 *>(d_out_images), stats, nullptr, nullptr, nullptr,
                           n_views > 1 ? &views : nullptr);
    if(rc == PT_OK) {
        PT_HIP(hipEventRecord(ev.e, s->stream));
        PT_HIP(hipStreamWaitEvent(caller, ev.e, 0));
        if(stats == nullptr && env_int("PT_VERIFY", 0) != 0) {
            rc = finish_path(s);
        }
    }
    return rc;
}

} // extern "C"

// ---- resumable frames (pt_frame_*) -----------------------------------------------------------------------------------------------
// A frame is a pt_render_tiles_ctl job that keeps what a stop leaves: per replica, the status of every stream after a launch, the park
// records of the streams a stop dropped with samples taken, the work list of the next launch (pt_frame.hip builds it from the status:
// parked streams first, then the untouched ones) and the count of unfinished pixels per tile.  The work list and the park records come in
// pairs that swap on every launch: a launch reads one and writes the other.

struct pt_frame {
    struct Replica {
        pt_scene *s = nullptr;
        std::vector<pt_tile> tiles; // its tiles, in the frame's order ...
        std::vector<size_t> index;  // ... and where they are in the frame's list
        uint32_t n_streams = 0;
        uint32_t n_todo = 0, n_parked = 0; // the next launch's work list: its length, and the parked streams at its head
        uint64_t samples_carried = 0, with_candidates = 0;
        uint32_t n_at_target = 0;                 // streams of the list at or above the target of the last progressive pass
        int32_t min_samples = 0, max_samples = 0; // samples taken, over the list's pixels
        bool ready = false; // the device tables exist
        bool in_order = true; // the work list is every stream of the replica in order (stream i at index i)
        int cur = 0;        // todo[cur] and park[cur] are what the next launch reads
        DevBuf<int4> d_tiles;
        DevBuf<uint32_t> d_offset, d_left, d_status, d_blocks, d_park_count;
        DevBuf<uint2> d_todo[2];
        DevBuf<PtParkRecord> d_park[2];
        DevBuf<unsigned long long> d_result;
        DevBuf<PtViewCamera> d_view_cams; // a view frame's tables
        DevBuf<uint64_t> d_view_seeds;
        // pt_frame_preview: the replica's gathered work list; on replica 0 also the frame's view and sample counts, which pixels a tile
        // covers, the frame's first-hit features and the other replicas' entries on their way in
        DevBuf<F4> pv_rgba, pv_view, pv_features, pv_stage_rgba;
        DevBuf<int2> pv_at, pv_stage_at;
        DevBuf<int32_t> pv_samples;
        DevBuf<uint8_t> pv_cover;
        bool pv_cover_ready = false, pv_features_ready = false;
        bool previewed = false; // device buffers of the preview exist
    };
    pt_camera_params camera{};
    pt_options options{};
    std::vector<pt_tile> tiles;
    uint64_t base_seed = 0;
    // a frame over a view batch (pt_frame_create_views, V > 1): the image is the V frames stacked, `views` the frame's own copy of the
    // cameras and seeds (every replica keeps them in device tables of its own: the scene's are any other batch's to overwrite between two
    // slices) and `cameras` what the preview's feature pass takes.  A plain frame has n_views = 1 and no tables.
    int32_t n_views = 1;
    ViewSet views;
    std::vector<pt_camera_params> cameras;
    int32_t rows() const { return n_views * options.image_height; }
    std::vector<std::unique_ptr<Replica>> reps;
    std::vector<uint8_t> tile_done;
    uint64_t tiles_done = 0, streams_total = 0;
    int32_t launches = 0;
    // progressive mode (pt_frame_set_progressive): passes of `quantum` samples per pixel; `target` is the sample count of the pass in
    // progress or last completed, the same for every replica
    int32_t quantum = 0, max_passes_per_call = 0, passes_completed = 0, target = 0;
    bool pass_in_progress = false;
    uint64_t samples_lost = 0;
    int status = PT_OK; // a failed frame returns this (and `error`) from every later call
    std::string error;
    mutable std::mutex mutex; // one call at a time
};

namespace {

// The device tables of a replica, made by its first launch: the tile table, the first stream of every tile and its pixel count, the
// status of every stream (all untouched) and the first work list (every stream, none parked).
int frame_prepare(pt_frame::Replica &r) {
    const size_t n_tiles = r.tiles.size();
    std::vector<int4> rects(n_tiles);
    std::vector<uint32_t> offsets(n_tiles), left(n_tiles);
    uint32_t at = 0;
    for(size_t k = 0; k < n_tiles; k++) {
        const pt_tile &t = r.tiles[k];
        rects[k] = make_int4(t.x, t.y, t.w, t.h);
        offsets[k] = at;
        left[k] = static_cast<uint32_t>(t.w) * static_cast<uint32_t>(t.h);
        at += left[k];
    }
    std::vector<uint2> todo(r.n_streams);
    for(uint32_t i = 0; i < r.n_streams; i++) {
        todo[i] = make_uint2(i, PT_NO_PARK);
    }
    PT_HIP(r.d_tiles.upload(rects));
    PT_HIP(r.d_offset.upload(offsets));
    PT_HIP(r.d_left.upload(left));
    PT_HIP(r.d_todo[0].upload(todo));
    PT_HIP(r.d_todo[1].ensure(r.n_streams));
    PT_HIP(r.d_status.ensure(r.n_streams));
    PT_HIP(hipMemset(r.d_status.ptr, 0, static_cast<size_t>(r.n_streams) * sizeof(uint32_t)));
    PT_HIP(r.d_blocks.ensure(2 * ((static_cast<size_t>(r.n_streams) + 1023) / 1024)));
    PT_HIP(r.d_park_count.ensure(1));
    PT_HIP(r.d_park[0].ensure(1));
    PT_HIP(r.d_result.ensure(16));
    r.ready = true;
    return PT_OK;
}

// The rectangles of the replica's unfinished tiles between the caller's image and the scene's frame in HBM
int frame_copy_open_tiles(const pt_frame &f, const pt_frame::Replica &r, float *out_image, bool to_device) {
    const size_t width = static_cast<size_t>(f.options.image_width);
    pt_scene *s = r.s;
    for(size_t k = 0; k < r.tiles.size(); k++) {
        if(f.tile_done[r.index[k]] != 0) {
            continue;
        }
        const pt_tile &t = r.tiles[k];
        const size_t at = static_cast<size_t>(t.y) * width + static_cast<size_t>(t.x);
        if(to_device) {
            PT_HIP(hipMemcpy2DAsync(s->image.ptr + at, width * sizeof(F4), out_image + at * 4, width * sizeof(F4), static_cast<size_t>(t.w) * sizeof(F4),
                                    static_cast<size_t>(t.h), hipMemcpyHostToDevice, s->stream));
        }
        else {
            PT_HIP(hipMemcpy2DAsync(out_image + at * 4, width * sizeof(F4), s->image.ptr + at, width * sizeof(F4), static_cast<size_t>(t.w) * sizeof(F4),
                                    static_cast<size_t>(t.h), hipMemcpyDeviceToHost, s->stream));
        }
    }
    return PT_OK;
}

// What one replica's launch of pt_frame_render did
struct FrameLaunch {
    StreamTally tally;
    uint64_t parked = 0; // streams it parked
};

// One launch of a replica: its work list, under the scene's lock, then the next work list
// (yield_at > 0: a pass of a progressive frame up to that sample count)
int frame_launch(pt_frame &f, pt_frame::Replica &r, float *out_image, pt_stats *stats, pt_progress_fn progress, void *progress_user, RenderStop *stop,
                 FrameLaunch *out, int32_t yield_at) {
    pt_scene *s = r.s;
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtDevOptions opt;
    int rc = derive_options(&f.options, &opt);
    if(rc != PT_OK) {
        return rc;
    }
    const PtDevCamera cam = derive_camera(&f.camera);
    if(!r.ready) {
        if(f.n_views > 1) {
            PT_HIP(r.d_view_cams.upload(f.views.cams));
            PT_HIP(r.d_view_seeds.upload(f.views.seeds));
        }
        rc = frame_prepare(r);
        if(rc != PT_OK) {
            return rc;
        }
    }
    const size_t pixels = static_cast<size_t>(f.options.image_width) * static_cast<size_t>(f.rows());
    PT_HIP(s->image.ensure(pixels));
    rc = frame_copy_open_tiles(f, r, out_image, true);
    if(rc != PT_OK) {
        return rc;
    }
    // park storage: one record per slot at most (a stop closes the pool, so a slot drops one stream at most), and never more than the streams left.
    // A progressive pass keeps the pool open and every stream of the list leaves a record, written by the launch or carried over: one per entry.
    PtPathConfig cfg;
    rc = ensure_path_workspace(s, r.n_todo, &cfg);
    if(rc != PT_OK) {
        return rc;
    }
    const int cur = r.cur, next = cur ^ 1;
    const bool progressive = yield_at > 0;
    const uint32_t cap = progressive ? r.n_todo : std::min<uint32_t>(r.n_todo, s->path_slots);
    if(progressive) {
        opt.overlap_bound = std::min(opt.max_sample_count, yield_at); // (the sample that reaches the target ends at a boundary of its own)
    }
    PT_HIP(r.d_park[next].ensure(cap));
    PT_HIP(hipMemsetAsync(r.d_park_count.ptr, 0, sizeof(uint32_t), s->stream));
    PtStreams T{};
    T.n = r.n_todo;
    T.tiles = r.d_tiles.ptr;
    T.tile_offset = r.d_offset.ptr;
    T.n_tiles = static_cast<uint32_t>(r.tiles.size());
    T.base_seed = f.base_seed;
    if(f.n_views > 1) {
        T.n_views = static_cast<uint32_t>(f.n_views);
        T.view_height = static_cast<uint32_t>(f.options.image_height);
        T.views = r.d_view_cams.ptr;
        T.view_seed = r.d_view_seeds.ptr;
    }
    // The first round is spread over the work list.  The first launch's list is every stream in order, so it is spread over the tile grid
    // as pt_render_tiles spreads it (an uninterrupted frame is scheduled exactly like one); a later list is no tile grid.
    T.tiles_per_row = 0;
    T.chunks_per_tile = 0;
    if(r.in_order) {
        tile_grid(r.tiles.data(), r.tiles.size(), &T.tiles_per_row, &T.chunks_per_tile);
    }
    T.tile_left = r.d_left.ptr;
    T.todo = r.d_todo[cur].ptr;
    T.park_in = r.d_park[cur].ptr;
    T.park_out = r.d_park[next].ptr;
    T.park_count = r.d_park_count.ptr;
    T.park_cap = cap;
    T.status = r.d_status.ptr;
    T.yield_at = progressive ? yield_at : 0;
    rc = run_path(s, cam, opt, T, reinterpret_cast<float4 *>(s->image.ptr), stats, progress, progress_user, nullptr, false, stop);
    if(rc != PT_OK) {
        return rc;
    }
    rc = frame_copy_open_tiles(f, r, out_image, false);
    if(rc != PT_OK) {
        return rc;
    }
    rc = finish_path(s, &out->tally);
    if(rc != PT_OK) {
        return rc;
    }
    if(pt_launch_frame_compact(s->stream, r.d_todo[cur].ptr, r.n_todo, r.d_status.ptr, r.d_park[next].ptr, r.d_todo[next].ptr, r.d_blocks.ptr, r.d_result.ptr,
                               progressive ? yield_at : 0, r.d_park[cur].ptr, r.d_park[next].ptr, r.d_park_count.ptr, cap) != 0) {
        PT_HIP(hipGetLastError());
        return fail(PT_ERR_HIP, "frame: work list kernel failed to launch");
    }
    unsigned long long res[16];
    PT_HIP(hipMemcpyAsync(res, r.d_result.ptr, sizeof(res), hipMemcpyDeviceToHost, s->stream));
    std::vector<uint32_t> left(r.tiles.size());
    PT_HIP(hipMemcpyAsync(left.data(), r.d_left.ptr, left.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    // every stream of the work list is finished, parked or still to do, and the stop dropped no more than the parked and returned ones
    const StreamTally &t = out->tally;
    // (res[8]: the records the launch wrote; a progressive pass drops no record: res[9], the samples of records that found no room, is 0)
    if(t.finished + res[0] + res[1] != r.n_todo || res[8] > t.abandoned || res[7] > cap || (!progressive && res[8] != res[0]) || res[9] != 0) {
        return fail(PT_ERR_HIP, "frame: " + std::to_string(t.finished) + " finished, " + std::to_string(res[0]) + " parked and " + std::to_string(res[1]) +
                                    " left of " + std::to_string(r.n_todo) + " streams (" + std::to_string(t.abandoned) + " dropped)");
    }
    r.n_todo = static_cast<uint32_t>(res[0] + res[1]);
    r.n_parked = static_cast<uint32_t>(res[7]);
    r.in_order = r.n_todo == r.n_streams && (r.n_parked == 0 || r.n_parked == r.n_todo) && (!progressive || res[0] == 0 || res[1] == 0); // (each part in order)
    r.samples_carried = res[3];
    r.with_candidates = res[4];
    r.n_at_target = progressive ? static_cast<uint32_t>(res[1]) : 0;
    r.min_samples = r.n_todo != 0 ? static_cast<int32_t>(0xffffffffULL - res[5]) : 0;
    r.max_samples = static_cast<int32_t>(res[6]);
    r.cur = next;
    out->parked = res[8];
    for(size_t k = 0; k < left.size(); k++) {
        f.tile_done[r.index[k]] = left[k] == 0 ? 1 : 0;
    }
    return PT_OK;
}

} // namespace

// pt_frame_create; `views` (a batch of more than one view, else null) makes it a frame over the stacked image, whose tiles lie in views->rows
static int frame_create_impl(pt_scene *const *scenes, int n_scenes, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles,
                             uint64_t base_seed, const ViewSet *views, pt_frame **out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null frame pointer");
    }
    *out = nullptr;
    if(scenes == nullptr || n_scenes < 1) {
        return fail(PT_ERR_INVALID, "no scenes");
    }
    for(int i = 0; i < n_scenes; i++) {
        if(scenes[i] == nullptr) {
            return fail(PT_ERR_INVALID, "null scene");
        }
    }
    if(camera == nullptr || options == nullptr || (tiles == nullptr && n_tiles > 0)) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(options->image_width <= 0 || options->image_height <= 0) {
        return fail(PT_ERR_INVALID, "image size must be positive");
    }
    const int32_t rows = views != nullptr ? views->rows(options) : options->image_height;
    uint64_t total = 0;
    for(size_t k = 0; k < n_tiles; k++) {
        const pt_tile &t = tiles[k];
        if(t.w <= 0 || t.h <= 0 || t.x < 0 || t.y < 0 || t.x + t.w > options->image_width || t.y + t.h > rows) {
            return fail(PT_ERR_INVALID, "tile outside the image or empty");
        }
        total += static_cast<uint64_t>(t.w) * static_cast<uint64_t>(t.h);
    }
    if(total > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "too many pixels in one frame");
    }
    PtDevOptions opt;
    const int rc = derive_options(options, &opt);
    if(rc != PT_OK) {
        return rc;
    }
    if(device_count_quiet() < 1) {
        return fail(PT_ERR_NO_DEVICE, "pt_frame_create: no HIP device (a frame renders on the GPU only)");
    }
    std::unique_ptr<pt_frame> f(new pt_frame());
    f->camera = *camera;
    f->options = *options;
    f->tiles.assign(tiles, tiles + n_tiles);
    f->base_seed = base_seed;
    if(views != nullptr) {
        f->n_views = static_cast<int32_t>(views->cams.size());
        f->views = *views;
        f->cameras.assign(camera, camera + f->n_views);
    }
    f->tile_done.assign(n_tiles, 0);
    f->streams_total = total;
    for(int i = 0; i < n_scenes; i++) {
        f->reps.emplace_back(new pt_frame::Replica());
        f->reps.back()->s = scenes[i];
    }
    const std::vector<int> owners = n_tiles > 0 ? tile_owners(tiles, n_tiles, n_scenes) : std::vector<int>();
    for(size_t k = 0; k < n_tiles; k++) {
        pt_frame::Replica &r = *f->reps[static_cast<size_t>(owners[k])];
        r.tiles.push_back(tiles[k]);
        r.index.push_back(k);
        r.n_streams += static_cast<uint32_t>(tiles[k].w) * static_cast<uint32_t>(tiles[k].h);
    }
    for(auto &r : f->reps) {
        r->n_todo = r->n_streams;
    }
    *out = f.release();
    return PT_OK;
}

extern "C" {

int pt_frame_create(pt_scene *const *scenes, int n_scenes, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles,
                    uint64_t base_seed, pt_frame **out) {
    return frame_create_impl(scenes, n_scenes, camera, options, tiles, n_tiles, base_seed, nullptr, out);
}

int pt_frame_create_views(pt_scene *const *scenes, int n_scenes, const pt_camera_params *cameras, const uint64_t *base_seeds, int32_t n_views,
                          const pt_options *options, pt_frame **out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null frame pointer");
    }
    *out = nullptr;
    std::vector<pt_tile> tiles;
    ViewSet views;
    const int rc = prepare_views(cameras, base_seeds, n_views, options, &tiles, &views);
    if(rc != PT_OK) {
        return rc;
    }
    // (one view: pt_frame_create over pt_job_tiles with its seed -- no view table, the same launches)
    return frame_create_impl(scenes, n_scenes, cameras, options, tiles.data(), tiles.size(), base_seeds[0], n_views > 1 ? &views : nullptr, out);
}

int pt_frame_render(pt_frame *f, float *out_image, pt_stats *stats, pt_progress_fn progress, void *progress_user, pt_render_control *ctl) {
    const RenderStop::Clock::time_point start = RenderStop::Clock::now();
    if(f == nullptr) {
        return fail(PT_ERR_INVALID, "null frame");
    }
    std::lock_guard<std::mutex> frame_lock(f->mutex);
    if(f->status != PT_OK) {
        return fail(f->status, f->error);
    }
    const int n_scenes = static_cast<int>(f->reps.size());
    if(stats != nullptr) {
        std::memset(stats, 0, sizeof(*stats) * static_cast<size_t>(n_scenes));
    }
    if(ctl != nullptr) {
        ctl->streams_finished = ctl->streams_abandoned = ctl->streams_unclaimed = 0;
        ctl->drain_ms = 0.0;
    }
    auto report_tiles = [&]() {
        if(ctl != nullptr && ctl->tile_done != nullptr && !f->tile_done.empty()) {
            std::memcpy(ctl->tile_done, f->tile_done.data(), f->tile_done.size());
        }
    };
    bool complete = true;
    for(const auto &r : f->reps) {
        complete = complete && r->n_todo == 0;
    }
    if(complete) {
        report_tiles();
        return PT_OK;
    }
    if(out_image == nullptr) {
        return fail(PT_ERR_INVALID, "null image");
    }
    pt_render_control none{};
    RenderStop stop;
    stop.ctl = ctl != nullptr ? ctl : &none;
    if(ctl != nullptr && ctl->budget_ms > 0.0) {
        stop.has_deadline = true;
        stop.deadline = start + std::chrono::duration_cast<RenderStop::Clock::duration>(std::chrono::duration<double, std::milli>(ctl->budget_ms));
    }
    stop.poll();
    // progress over the whole frame, serialised over the replicas (as pt_render_tiles_multi)
    struct Shared {
        std::mutex mutex;
        int completed = 0, total = 0;
        pt_progress_fn fn = nullptr;
        void *user = nullptr;
    } shared;
    shared.completed = static_cast<int>(f->tiles_done);
    shared.total = static_cast<int>(f->tiles.size());
    shared.fn = progress;
    shared.user = progress_user;
    auto trampoline = [](int, int, void *p) {
        Shared *sh = static_cast<Shared *>(p);
        std::lock_guard<std::mutex> lock(sh->mutex);
        sh->completed++;
        sh->fn(sh->completed, sh->total, sh->user);
    };
    // A plain frame makes one launch per replica that has work.  A progressive frame makes one per pass: every replica runs the pass over its
    // own tiles up to the frame's target, and the next pass starts when all of them have ended theirs.
    uint64_t left = 0, parked = 0;
    int passes_this_call = 0;
    bool pass_limit = false;
    std::vector<pt_stats> pass_stats(stats != nullptr ? static_cast<size_t>(n_scenes) : 0);
    for(;;) {
        int32_t yield_at = 0;
        if(f->quantum > 0) {
            if(!f->pass_in_progress) {
                f->target = f->target > INT32_MAX - f->quantum ? INT32_MAX : f->target + f->quantum;
                f->pass_in_progress = true;
            }
            yield_at = f->target;
        }
        std::vector<int> rcs(static_cast<size_t>(n_scenes), PT_OK);
        std::vector<std::string> errors(static_cast<size_t>(n_scenes));
        std::vector<FrameLaunch> launched(static_cast<size_t>(n_scenes));
        std::vector<char> ran(static_cast<size_t>(n_scenes), 0);
        if(stats != nullptr) {
            std::memset(pass_stats.data(), 0, sizeof(pt_stats) * pass_stats.size());
        }
        auto work = [&](int i) {
            pt_frame::Replica &r = *f->reps[static_cast<size_t>(i)];
            if(r.n_todo == 0) {
                return;
            }
            ran[static_cast<size_t>(i)] = 1;
            rcs[static_cast<size_t>(i)] = frame_launch(*f, r, out_image, stats != nullptr ? &pass_stats[static_cast<size_t>(i)] : nullptr,
                                                       progress != nullptr ? static_cast<pt_progress_fn>(trampoline) : nullptr, &shared, &stop, &launched[static_cast<size_t>(i)], yield_at);
            if(rcs[static_cast<size_t>(i)] != PT_OK) {
                errors[static_cast<size_t>(i)] = g_last_error;
            }
        };
        std::vector<std::thread> threads;
        for(int i = 1; i < n_scenes; i++) {
            threads.emplace_back(work, i);
        }
        work(0);
        for(std::thread &t : threads) {
            t.join();
        }
        for(int i = 0; i < n_scenes; i++) {
            f->launches += ran[static_cast<size_t>(i)];
        }
        for(int i = 0; i < n_scenes; i++) {
            if(rcs[static_cast<size_t>(i)] != PT_OK) {
                f->status = rcs[static_cast<size_t>(i)];
                f->error = "frame failed: scene " + std::to_string(i) + ": " + errors[static_cast<size_t>(i)];
                return fail(f->status, f->error);
            }
        }
        f->tiles_done = static_cast<uint64_t>(std::count(f->tile_done.begin(), f->tile_done.end(), 1));
        left = 0;
        parked = 0;
        uint64_t at_target = 0;
        if(ctl != nullptr) {
            ctl->streams_abandoned = ctl->streams_unclaimed = 0; // (of the call's last launches)
        }
        for(int i = 0; i < n_scenes; i++) {
            const FrameLaunch &l = launched[static_cast<size_t>(i)];
            left += f->reps[static_cast<size_t>(i)]->n_todo;
            at_target += f->reps[static_cast<size_t>(i)]->n_at_target;
            parked += l.parked;
            if(ctl != nullptr) {
                ctl->streams_finished += l.tally.finished;
                ctl->streams_abandoned += l.parked;
                ctl->streams_unclaimed += l.tally.unclaimed + (l.tally.abandoned - l.parked); // (dropped before their first sample: they start afresh)
            }
            if(stats != nullptr) {
                // the work of all the call's launches; the grid is the last launch's
                const pt_stats &p = pass_stats[static_cast<size_t>(i)];
                pt_stats &o = stats[i];
                o.samples += p.samples;
                o.rays_traced += p.rays_traced;
                o.shadow_rays_traced += p.shadow_rays_traced;
                o.node_visits += p.node_visits;
                o.leaf_tests += p.leaf_tests;
                o.vertices += p.vertices;
                o.launches += p.launches;
                o.kernel_ms += p.kernel_ms;
                o.wave_steps += p.wave_steps;
                o.shading_passes += p.shading_passes;
                if(p.launches != 0) {
                    o.wavefronts = p.wavefronts;
                    o.slot_rows = p.slot_rows;
                }
            }
        }
        if(yield_at == 0) {
            break;
        }
        // the pass has ended when every stream that is left has its samples (a stop that came too late to drop anything ends it too)
        const bool pass_done = at_target == left;
        if(pass_done) {
            f->pass_in_progress = false;
            f->passes_completed++;
            passes_this_call++;
        }
        if(left == 0 || !pass_done) {
            break;
        }
        stop.poll();
        if(stop.requested.load()) {
            break;
        }
        if(f->max_passes_per_call > 0 && passes_this_call >= f->max_passes_per_call) {
            pass_limit = true;
            break;
        }
    }
    report_tiles();
    if(ctl != nullptr) {
        ctl->drain_ms = stop.drain_ms;
    }
    if(left != 0) {
        const std::string why = pass_limit ? "pass limit reached" : (__atomic_load_n(&stop.ctl->cancel, __ATOMIC_ACQUIRE) != 0 ? "cancelled" : "budget spent");
        return fail(PT_ERR_CANCELLED, "frame stopped (" + why + "): " + std::to_string(parked) + " streams parked, " + std::to_string(left) + " streams left");
    }
    return PT_OK;
}

int pt_frame_set_progressive(pt_frame *f, int32_t quantum, int32_t max_passes_per_call) {
    if(f == nullptr) {
        return fail(PT_ERR_INVALID, "null frame");
    }
    if(quantum < 0) {
        return fail(PT_ERR_INVALID, "negative quantum");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    if(f->status != PT_OK) {
        return fail(f->status, f->error);
    }
    f->quantum = quantum;
    f->max_passes_per_call = std::max(max_passes_per_call, 0);
    if(quantum == 0) {
        f->pass_in_progress = false; // (what an interrupted pass left is a plain frame's work now)
    }
    return PT_OK;
}

int pt_frame_get_progress(const pt_frame *f, pt_frame_progress *out) {
    if(f == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    if(f->status != PT_OK) {
        return fail(f->status, f->error);
    }
    std::memset(out, 0, sizeof(*out));
    out->quantum = f->quantum;
    out->max_passes_per_call = f->max_passes_per_call;
    out->passes_completed = f->passes_completed;
    out->target = f->target;
    out->pass_in_progress = f->pass_in_progress ? 1 : 0;
    bool any = false;
    for(const auto &r : f->reps) {
        if(r->n_todo == 0) {
            continue;
        }
        out->min_samples = any ? std::min(out->min_samples, r->min_samples) : r->min_samples;
        out->max_samples = any ? std::max(out->max_samples, r->max_samples) : r->max_samples;
        out->streams_at_target += r->n_at_target;
        any = true;
    }
    out->samples_lost = f->samples_lost;
    return PT_OK;
}

int pt_frame_get_info(const pt_frame *f, pt_frame_info *info) {
    if(f == nullptr || info == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    std::memset(info, 0, sizeof(*info));
    info->streams_total = f->streams_total;
    info->tiles_total = f->tiles.size();
    info->tiles_done = f->tiles_done;
    for(const auto &r : f->reps) {
        info->streams_parked += r->n_parked;
        info->streams_untouched += r->n_todo - r->n_parked;
        info->samples_carried += r->samples_carried;
        info->parked_with_candidates += r->with_candidates;
        info->park_bytes += (r->d_park[0].count + r->d_park[1].count) * sizeof(PtParkRecord);
    }
    info->streams_finished = f->streams_total - info->streams_parked - info->streams_untouched;
    info->launches = f->launches;
    info->status = f->status;
    return PT_OK;
}

int pt_frame_destroy(pt_frame *f) {
    if(f == nullptr) {
        return fail(PT_ERR_INVALID, "null frame");
    }
    {
        std::lock_guard<std::mutex> frame_lock(f->mutex);
        for(auto &r : f->reps) {
            // (the buffers go on the scene's device, and not while the scene's stream may still use them)
            std::lock_guard<std::mutex> lock(r->s->render_mutex);
            if(r->ready || r->previewed || r->d_park[0].ptr != nullptr || r->d_park[1].ptr != nullptr) {
                (void)hipSetDevice(r->s->device);
                (void)hipStreamSynchronize(r->s->stream);
            }
            r.reset();
        }
    }
    delete f;
    return PT_OK;
}

} // extern "C"

// ---- post-processing (pt_post.hip) ----------------------------------------------------------------------------------------------

static int post_check(int device, const float *rgba, int32_t width, int32_t height, uint32_t steps, float gamma) {
    if(width < 0 || height < 0 || (rgba == nullptr && static_cast<long long>(width) * height > 0)) {
        return fail(PT_ERR_INVALID, "bad image");
    }
    if((steps & ~(PT_POST_TONE_MAP | PT_POST_GAMMA)) != 0 || steps == 0) {
        return fail(PT_ERR_INVALID, "steps must be PT_POST_TONE_MAP and/or PT_POST_GAMMA");
    }
    if((steps & PT_POST_GAMMA) != 0 && !(gamma == gamma)) {
        return fail(PT_ERR_INVALID, "gamma is NaN");
    }
    const int n_dev = device_count_quiet();
    if(n_dev <= 0) {
        return fail(PT_ERR_NO_DEVICE, "no HIP device available; libpathtrace_hip has no CPU path");
    }
    if(device < 0 || device >= n_dev) {
        return fail(PT_ERR_NO_DEVICE, "device index out of range");
    }
    return PT_OK;
}

int pt_post_process_device(int device, float *d_rgba, int32_t width, int32_t height, uint32_t steps, float gamma, void *stream) {
    const int rc = post_check(device, d_rgba, width, height, steps, gamma);
    if(rc != PT_OK) {
        return rc;
    }
    PT_HIP(hipSetDevice(device));
    static_assert(PT_POST_TONE_MAP == PT_POST_STEP_TONE_MAP && PT_POST_GAMMA == PT_POST_STEP_GAMMA, "step bits");
    PT_HIP(pt_post_run(static_cast<hipStream_t>(stream), reinterpret_cast<float4 *>(d_rgba), width, height, steps, gamma));
    return PT_OK;
}

int pt_post_process(int device, float *rgba, int32_t width, int32_t height, uint32_t steps, float gamma) {
    const int rc = post_check(device, rgba, width, height, steps, gamma);
    if(rc != PT_OK) {
        return rc;
    }
    const size_t count = static_cast<size_t>(width) * static_cast<size_t>(height);
    if(count == 0) {
        return PT_OK;
    }
    PT_HIP(hipSetDevice(device));
    DevBuf<F4> frame;
    PT_HIP(frame.ensure(count));
    PT_HIP(hipMemcpy(frame.ptr, rgba, count * sizeof(F4), hipMemcpyHostToDevice));
    PT_HIP(pt_post_run(nullptr, reinterpret_cast<float4 *>(frame.ptr), width, height, steps, gamma));
    PT_HIP(hipMemcpy(rgba, frame.ptr, count * sizeof(F4), hipMemcpyDeviceToHost));
    return PT_OK;
}

// ---- feature-guided denoising (pt_path.hip: pt_feature_kernel; pt_denoise.hip) -------------------------------------------------------

static int features_check(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const float *out) {
    int rc = check_render_args(s, camera, options);
    if(rc != PT_OK) {
        return rc;
    }
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(static_cast<long long>(options->image_width) * options->image_height > 0x0fffffffLL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    return PT_OK;
}

// Enqueues the feature pass on the scene's stream (render_mutex held): into `d_out`, width * height * 3 float4.
static int features_launch(pt_scene *s, const pt_camera_params *camera, const pt_options *options, float4 *d_out) {
    int rc = setup_path(s);
    if(rc != PT_OK) {
        return rc;
    }
    PtDevCamera cam = derive_camera(camera);
    cam.aperture_kind = PT_APERTURE_NONE; // the rays are a pure function of camera and pixel
    PtPathConfig cfg = s->path_cfg;
    const size_t n = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    PT_HIP(s->feature_spill.ensure(((n + 255) / 256) * 256 * cfg.spill_depth));
    cfg.spill = s->feature_spill.ptr;
    pt_launch_features(s->stream, s->dev, cam, options->image_width, options->image_height, d_out, cfg);
    PT_HIP(hipGetLastError());
    return PT_OK;
}

// The arguments of the view forms (pt_render_features_views*), checked without a device
static int features_views_check(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, const float *out) {
    if(n_views <= 0) {
        return fail(PT_ERR_INVALID, "a view batch needs at least one view");
    }
    if(options != nullptr && options->image_width > 0 && options->image_height > 0 &&
       static_cast<uint64_t>(n_views) * static_cast<uint64_t>(options->image_height) * static_cast<uint64_t>(options->image_width) > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    return features_check(s, cameras, options, out);
}

// features_launch for the stacked frames of n_views cameras, in one launch: into `d_out`, n_views * width * height * 3 float4.
static int features_views_launch(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, float4 *d_out) {
    if(n_views == 1) {
        return features_launch(s, cameras, options, d_out);
    }
    int rc = setup_path(s);
    if(rc != PT_OK) {
        return rc;
    }
    std::vector<PtViewCamera> table(static_cast<size_t>(n_views));
    for(int32_t v = 0; v < n_views; v++) {
        table[static_cast<size_t>(v)] = PtViewCamera{derive_camera(cameras + v), {0, 0, 0}};
        table[static_cast<size_t>(v)].cam.aperture_kind = PT_APERTURE_NONE; // the rays are a pure function of camera and pixel
    }
    PT_HIP(s->feature_cams.ensure(table.size()));
    PT_HIP(hipMemcpyAsync(s->feature_cams.ptr, table.data(), table.size() * sizeof(PtViewCamera), hipMemcpyHostToDevice, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream)); // the table is this function's vector
    PtPathConfig cfg = s->path_cfg;
    const size_t n = static_cast<size_t>(n_views) * static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    PT_HIP(s->feature_spill.ensure(((n + 255) / 256) * 256 * cfg.spill_depth));
    cfg.spill = s->feature_spill.ptr;
    pt_launch_features_views(s->stream, s->dev, s->feature_cams.ptr, n_views, options->image_width, options->image_height, d_out, cfg);
    PT_HIP(hipGetLastError());
    return PT_OK;
}

namespace {

// The denoiser's scratch buffers: one set per device, grown on demand, one call at a time per device.  They live as long as the process
// (never freed: a static destructor would run after the HIP runtime has gone).
struct DenoiseWorkspace {
    std::mutex mutex;
    size_t pixels = 0;  // capacity of the per-pixel buffers
    size_t staged = 0;  // ... and of the host form's upload/download buffers
    PtDenoiseScratch scratch{};
    float4 *in_rgba = nullptr, *in_features = nullptr;
};

DenoiseWorkspace &denoise_workspace(int device) {
    static std::mutex table_mutex;
    static std::vector<DenoiseWorkspace *> table;
    std::lock_guard<std::mutex> lock(table_mutex);
    if(static_cast<size_t>(device) >= table.size()) {
        table.resize(static_cast<size_t>(device) + 1, nullptr);
    }
    if(table[static_cast<size_t>(device)] == nullptr) {
        table[static_cast<size_t>(device)] = new DenoiseWorkspace();
    }
    return *table[static_cast<size_t>(device)];
}

template<typename T>
hipError_t regrow(T **p, size_t count) {
    if(*p != nullptr) {
        hipError_t e = hipFree(*p);
        *p = nullptr;
        if(e != hipSuccess) {
            return e;
        }
    }
    return hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(count, 1) * sizeof(T));
}

int denoise_ensure(DenoiseWorkspace &ws, size_t n, bool staged) {
    PtDenoiseScratch &d = ws.scratch;
    if(n > ws.pixels) {
        ws.pixels = 0;
        PT_HIP(regrow(&d.col[0], n));
        PT_HIP(regrow(&d.col[1], n));
        PT_HIP(regrow(&d.var[0], n));
        PT_HIP(regrow(&d.var[1], n));
        PT_HIP(regrow(&d.guide, n));
        PT_HIP(regrow(&d.grad, n));
        PT_HIP(regrow(&d.cls, n));
        ws.pixels = n;
    }
    if(staged && n > ws.staged) {
        ws.staged = 0;
        PT_HIP(regrow(&ws.in_rgba, n));
        PT_HIP(regrow(&ws.in_features, 3 * n));
        ws.staged = n;
    }
    return PT_OK;
}

// The parameters pt_denoise takes (NULL = the defaults), checked without a device
int denoise_params_resolve(const pt_denoise_params *params, PtDenoiseParams *resolved) {
    pt_denoise_params p{};
    pt_denoise_params_default(&p);
    if(params != nullptr) {
        p = *params;
    }
    if(p.iterations < 0 || p.iterations > 10) {
        return fail(PT_ERR_INVALID, "iterations must be 0..10");
    }
    for(float sigma : {p.sigma_luminance, p.sigma_normal, p.sigma_depth}) {
        if(!std::isfinite(sigma) || sigma < 0.0F) {
            return fail(PT_ERR_INVALID, "sigmas must be finite and not negative");
        }
    }
    *resolved = PtDenoiseParams{p.iterations, p.sigma_luminance, p.sigma_normal, p.sigma_depth};
    return PT_OK;
}

int denoise_check(int device, const void *rgba, const void *features, int32_t width, int32_t height, const pt_denoise_params *params, const void *out,
                  PtDenoiseParams *resolved) {
    if(rgba == nullptr || features == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(width <= 0 || height <= 0) {
        return fail(PT_ERR_INVALID, "image size must be positive");
    }
    if(static_cast<long long>(width) * height > 0x0fffffffLL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    PtDenoiseParams p{};
    const int rc = denoise_params_resolve(params, &p);
    if(rc != PT_OK) {
        return rc;
    }
    const int n_dev = device_count_quiet();
    if(n_dev <= 0) {
        return fail(PT_ERR_NO_DEVICE, "no HIP device available; libpathtrace_hip has no CPU path");
    }
    if(device < 0 || device >= n_dev) {
        return fail(PT_ERR_NO_DEVICE, "device index out of range");
    }
    *resolved = p;
    return PT_OK;
}

} // namespace

extern "C" {

int pt_denoise_params_default(pt_denoise_params *out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    out->iterations = 5;
    out->sigma_luminance = 32.0F;
    out->sigma_normal = 128.0F;
    out->sigma_depth = 1.0F;
    return PT_OK;
}

int pt_render_features(pt_scene *s, const pt_camera_params *camera, const pt_options *options, float *out_features) {
    int rc = features_check(s, camera, options, out_features);
    if(rc != PT_OK) {
        return rc;
    }
    const size_t n = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(s->features.ensure(3 * n));
    rc = features_launch(s, camera, options, reinterpret_cast<float4 *>(s->features.ptr));
    if(rc != PT_OK) {
        return rc;
    }
    PT_HIP(hipMemcpyAsync(out_features, s->features.ptr, 3 * n * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    return PT_OK;
}

int pt_render_features_device(pt_scene *s, const pt_camera_params *camera, const pt_options *options, float *d_out_features, void *stream) {
    int rc = features_check(s, camera, options, d_out_features);
    if(rc != PT_OK) {
        return rc;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    // order after the caller's stream, trace on the library's stream, then make the caller's stream wait for it
    hipStream_t caller = static_cast<hipStream_t>(stream);
    Event ev;
    PT_HIP(ev.create(hipEventDisableTiming));
    PT_HIP(hipEventRecord(ev.e, caller));
    PT_HIP(hipStreamWaitEvent(s->stream, ev.e, 0));
    rc = features_launch(s, camera, options, reinterpret_cast<float4 *>(d_out_features));
    if(rc != PT_OK) {
        return rc;
    }
    PT_HIP(hipEventRecord(ev.e, s->stream));
    PT_HIP(hipStreamWaitEvent(caller, ev.e, 0));
    if(caller == nullptr) {
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    return PT_OK;
}

int pt_render_features_views(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, float *out_features) {
    int rc = features_views_check(s, cameras, n_views, options, out_features);
    if(rc != PT_OK) {
        return rc;
    }
    const size_t n = static_cast<size_t>(n_views) * static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(s->features.ensure(3 * n));
    rc = features_views_launch(s, cameras, n_views, options, reinterpret_cast<float4 *>(s->features.ptr));
    if(rc != PT_OK) {
        return rc;
    }
    PT_HIP(hipMemcpyAsync(out_features, s->features.ptr, 3 * n * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    return PT_OK;
}

int pt_render_features_views_device(pt_scene *s, const pt_camera_params *cameras, int32_t n_views, const pt_options *options, float *d_out_features, void *stream) {
    int rc = features_views_check(s, cameras, n_views, options, d_out_features);
    if(rc != PT_OK) {
        return rc;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    // ordered as pt_render_features_device
    hipStream_t caller = static_cast<hipStream_t>(stream);
    Event ev;
    PT_HIP(ev.create(hipEventDisableTiming));
    PT_HIP(hipEventRecord(ev.e, caller));
    PT_HIP(hipStreamWaitEvent(s->stream, ev.e, 0));
    rc = features_views_launch(s, cameras, n_views, options, reinterpret_cast<float4 *>(d_out_features));
    if(rc != PT_OK) {
        return rc;
    }
    PT_HIP(hipEventRecord(ev.e, s->stream));
    PT_HIP(hipStreamWaitEvent(caller, ev.e, 0));
    if(caller == nullptr) {
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    return PT_OK;
}

int pt_denoise_device(int device, const float *d_rgba, const float *d_features, int32_t width, int32_t height, const pt_denoise_params *params, float *d_out_rgba,
                      void *stream) {
    PtDenoiseParams p{};
    int rc = denoise_check(device, d_rgba, d_features, width, height, params, d_out_rgba, &p);
    if(rc != PT_OK) {
        return rc;
    }
    const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
    DenoiseWorkspace &ws = denoise_workspace(device);
    std::lock_guard<std::mutex> lock(ws.mutex);
    PT_HIP(hipSetDevice(device));
    rc = denoise_ensure(ws, n, false);
    if(rc != PT_OK) {
        return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    PT_HIP(pt_denoise_run(st, reinterpret_cast<const float4 *>(d_rgba), reinterpret_cast<const float4 *>(d_features), width, height, p, ws.scratch,
                          reinterpret_cast<float4 *>(d_out_rgba)));
    PT_HIP(hipStreamSynchronize(st)); // the scratch buffers are the device's: the next call may reuse them
    return PT_OK;
}

int pt_denoise(int device, const float *rgba, const float *features, int32_t width, int32_t height, const pt_denoise_params *params, float *out_rgba) {
    PtDenoiseParams p{};
    int rc = denoise_check(device, rgba, features, width, height, params, out_rgba, &p);
    if(rc != PT_OK) {
        return rc;
    }
    const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
    DenoiseWorkspace &ws = denoise_workspace(device);
    std::lock_guard<std::mutex> lock(ws.mutex);
    PT_HIP(hipSetDevice(device));
    rc = denoise_ensure(ws, n, true);
    if(rc != PT_OK) {
        return rc;
    }
    PT_HIP(hipMemcpy(ws.in_rgba, rgba, n * sizeof(F4), hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(ws.in_features, features, 3 * n * sizeof(F4), hipMemcpyHostToDevice));
    // in place: the last kernel reads a pixel's alpha before it writes that pixel, and no kernel reads another pixel of the input
    PT_HIP(pt_denoise_run(nullptr, ws.in_rgba, ws.in_features, width, height, p, ws.scratch, ws.in_rgba));
    PT_HIP(hipMemcpy(out_rgba, ws.in_rgba, n * sizeof(F4), hipMemcpyDeviceToHost));
    return PT_OK;
}

// The view forms: n_views frames stacked, every stage one launch for all of them (pt_denoise_views_run)
static int denoise_views_check(int device, const void *rgba, const void *features, int32_t width, int32_t height, int32_t n_views, const pt_denoise_params *params,
                               const void *out, PtDenoiseParams *resolved) {
    if(n_views <= 0) {
        return fail(PT_ERR_INVALID, "a view batch needs at least one view");
    }
    if(width > 0 && height > 0 && static_cast<uint64_t>(n_views) * static_cast<uint64_t>(width) * static_cast<uint64_t>(height) > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    return denoise_check(device, rgba, features, width, height, params, out, resolved);
}

int pt_denoise_views_device(int device, const float *d_rgba, const float *d_features, int32_t width, int32_t height, int32_t n_views, const pt_denoise_params *params,
                            float *d_out_rgba, void *stream) {
    PtDenoiseParams p{};
    int rc = denoise_views_check(device, d_rgba, d_features, width, height, n_views, params, d_out_rgba, &p);
    if(rc != PT_OK) {
        return rc;
    }
    const size_t n = static_cast<size_t>(n_views) * static_cast<size_t>(width) * static_cast<size_t>(height);
    DenoiseWorkspace &ws = denoise_workspace(device);
    std::lock_guard<std::mutex> lock(ws.mutex);
    PT_HIP(hipSetDevice(device));
    rc = denoise_ensure(ws, n, false);
    if(rc != PT_OK) {
        return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    PT_HIP(pt_denoise_views_run(st, reinterpret_cast<const float4 *>(d_rgba), reinterpret_cast<const float4 *>(d_features), nullptr, width, height, n_views, p,
                                ws.scratch, reinterpret_cast<float4 *>(d_out_rgba)));
    PT_HIP(hipStreamSynchronize(st)); // the scratch buffers are the device's: the next call may reuse them
    return PT_OK;
}

int pt_denoise_views(int device, const float *rgba, const float *features, int32_t width, int32_t height, int32_t n_views, const pt_denoise_params *params,
                     float *out_rgba) {
    PtDenoiseParams p{};
    int rc = denoise_views_check(device, rgba, features, width, height, n_views, params, out_rgba, &p);
    if(rc != PT_OK) {
        return rc;
    }
    const size_t n = static_cast<size_t>(n_views) * static_cast<size_t>(width) * static_cast<size_t>(height);
    DenoiseWorkspace &ws = denoise_workspace(device);
    std::lock_guard<std::mutex> lock(ws.mutex);
    PT_HIP(hipSetDevice(device));
    rc = denoise_ensure(ws, n, true);
    if(rc != PT_OK) {
        return rc;
    }
    PT_HIP(hipMemcpy(ws.in_rgba, rgba, n * sizeof(F4), hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(ws.in_features, features, 3 * n * sizeof(F4), hipMemcpyHostToDevice));
    // in place, as pt_denoise
    PT_HIP(pt_denoise_views_run(nullptr, ws.in_rgba, ws.in_features, nullptr, width, height, n_views, p, ws.scratch, ws.in_rgba));
    PT_HIP(hipMemcpy(out_rgba, ws.in_rgba, n * sizeof(F4), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_frame_preview(pt_frame *f, const float *image, const pt_denoise_params *denoise, float *out_rgba, int32_t *out_samples) {
    if(f == nullptr || image == nullptr || out_rgba == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    PtDenoiseParams dp{};
    if(denoise != nullptr) {
        const int rc = denoise_params_resolve(denoise, &dp);
        if(rc != PT_OK) {
            return rc;
        }
    }
    // (a view frame's image is its views stacked: every step below but the features and the filter sees one frame of rows() rows)
    const int32_t width = f->options.image_width, height = f->options.image_height;
    const size_t n = static_cast<size_t>(width) * static_cast<size_t>(f->rows());
    if(n > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    std::lock_guard<std::mutex> frame_lock(f->mutex);
    if(f->status != PT_OK) {
        return fail(f->status, f->error);
    }
    bool any_ready = false;
    for(const auto &r : f->reps) {
        any_ready = any_ready || r->ready;
    }
    if(!any_ready) {
        // before the first pt_frame_render every pixel is a hole, and a frame of holes stays one when it is filtered
        std::memset(out_rgba, 0, n * sizeof(F4));
        if(out_samples != nullptr) {
            std::memset(out_samples, 0, n * sizeof(int32_t));
        }
        return PT_OK;
    }
    // 1. every replica gathers its work list on its own device; the other replicas' entries come to the host
    const size_t n_reps = f->reps.size();
    std::vector<std::vector<F4>> far_rgba(n_reps);
    std::vector<std::vector<int2>> far_at(n_reps);
    for(size_t i = 0; i < n_reps; i++) {
        pt_frame::Replica &r = *f->reps[i];
        if(!r.ready || r.n_todo == 0) {
            continue;
        }
        pt_scene *s = r.s;
        std::lock_guard<std::mutex> lock(s->render_mutex);
        PT_HIP(hipSetDevice(s->device));
        r.previewed = true;
        PT_HIP(r.pv_rgba.ensure(r.n_todo));
        PT_HIP(r.pv_at.ensure(r.n_todo));
        if(pt_launch_frame_gather(s->stream, r.d_todo[r.cur].ptr, r.n_todo, r.n_parked, r.d_park[r.cur].ptr, r.d_tiles.ptr, r.d_offset.ptr,
                                  static_cast<uint32_t>(r.tiles.size()), width, reinterpret_cast<float4 *>(r.pv_rgba.ptr), r.pv_at.ptr) != 0) {
            PT_HIP(hipGetLastError());
            return fail(PT_ERR_HIP, "preview: gather kernel failed to launch");
        }
        if(i != 0) {
            far_rgba[i].resize(r.n_todo);
            far_at[i].resize(r.n_todo);
            PT_HIP(hipMemcpyAsync(far_rgba[i].data(), r.pv_rgba.ptr, r.n_todo * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
            PT_HIP(hipMemcpyAsync(far_at[i].data(), r.pv_at.ptr, r.n_todo * sizeof(int2), hipMemcpyDeviceToHost, s->stream));
            PT_HIP(hipStreamSynchronize(s->stream));
        }
    }
    // 2. replica 0's device: the caller's image, the holes no tile covers, every replica's entries over them; then the filter
    pt_frame::Replica &r0 = *f->reps[0];
    pt_scene *s0 = r0.s;
    std::lock_guard<std::mutex> lock(s0->render_mutex);
    PT_HIP(hipSetDevice(s0->device));
    hipStream_t st = s0->stream;
    r0.previewed = true;
    PT_HIP(r0.pv_view.ensure(n));
    PT_HIP(r0.pv_samples.ensure(n));
    if(!r0.pv_cover_ready) {
        std::vector<uint8_t> cover(n, 0);
        for(const pt_tile &t : f->tiles) {
            for(int32_t y = t.y; y < t.y + t.h; y++) {
                std::memset(cover.data() + static_cast<size_t>(y) * width + t.x, 1, static_cast<size_t>(t.w));
            }
        }
        PT_HIP(r0.pv_cover.upload(cover));
        r0.pv_cover_ready = true;
    }
    float4 *view = reinterpret_cast<float4 *>(r0.pv_view.ptr);
    PT_HIP(hipMemcpyAsync(view, image, n * sizeof(F4), hipMemcpyHostToDevice, st));
    if(pt_launch_frame_preview_base(st, view, r0.pv_samples.ptr, r0.pv_cover.ptr, static_cast<uint32_t>(n)) != 0) {
        PT_HIP(hipGetLastError());
        return fail(PT_ERR_HIP, "preview: base kernel failed to launch");
    }
    for(size_t i = 0; i < n_reps; i++) {
        const pt_frame::Replica &r = *f->reps[i];
        if(!r.ready) {
            // (no launch yet: every pixel of its tiles is a hole)
            for(const pt_tile &t : r.tiles) {
                const size_t at = static_cast<size_t>(t.y) * width + static_cast<size_t>(t.x);
                PT_HIP(hipMemset2DAsync(view + at, width * sizeof(F4), 0, static_cast<size_t>(t.w) * sizeof(F4), static_cast<size_t>(t.h), st));
                PT_HIP(hipMemset2DAsync(r0.pv_samples.ptr + at, width * sizeof(int32_t), 0, static_cast<size_t>(t.w) * sizeof(int32_t), static_cast<size_t>(t.h), st));
            }
            continue;
        }
        if(r.n_todo == 0) {
            continue;
        }
        const float4 *rgba = reinterpret_cast<const float4 *>(r0.pv_rgba.ptr);
        const int2 *at = r0.pv_at.ptr;
        if(i != 0) {
            PT_HIP(r0.pv_stage_rgba.ensure(r.n_todo));
            PT_HIP(r0.pv_stage_at.ensure(r.n_todo));
            PT_HIP(hipMemcpyAsync(r0.pv_stage_rgba.ptr, far_rgba[i].data(), r.n_todo * sizeof(F4), hipMemcpyHostToDevice, st));
            PT_HIP(hipMemcpyAsync(r0.pv_stage_at.ptr, far_at[i].data(), r.n_todo * sizeof(int2), hipMemcpyHostToDevice, st));
            rgba = reinterpret_cast<const float4 *>(r0.pv_stage_rgba.ptr);
            at = r0.pv_stage_at.ptr;
        }
        if(pt_launch_frame_scatter(st, rgba, at, r.n_todo, view, r0.pv_samples.ptr) != 0) {
            PT_HIP(hipGetLastError());
            return fail(PT_ERR_HIP, "preview: scatter kernel failed to launch");
        }
    }
    std::unique_lock<std::mutex> ws_lock;
    if(denoise != nullptr) {
        if(!r0.pv_features_ready) {
            PT_HIP(r0.pv_features.ensure(3 * n));
            const int rc = f->n_views > 1 ? features_views_launch(s0, f->cameras.data(), f->n_views, &f->options, reinterpret_cast<float4 *>(r0.pv_features.ptr))
                                          : features_launch(s0, &f->camera, &f->options, reinterpret_cast<float4 *>(r0.pv_features.ptr));
            if(rc != PT_OK) {
                return rc;
            }
            r0.pv_features_ready = true;
        }
        DenoiseWorkspace &ws = denoise_workspace(s0->device);
        ws_lock = std::unique_lock<std::mutex>(ws.mutex); // (held until the stream has been synchronised below)
        const int rc = denoise_ensure(ws, n, false);
        if(rc != PT_OK) {
            return rc;
        }
        // (one view: pt_denoise_masked_run itself; more: its view form, a hole filled from its own view only)
        PT_HIP(pt_denoise_views_run(st, view, reinterpret_cast<const float4 *>(r0.pv_features.ptr), r0.pv_samples.ptr, width, height, f->n_views, dp, ws.scratch, view));
    }
    PT_HIP(hipMemcpyAsync(out_rgba, view, n * sizeof(F4), hipMemcpyDeviceToHost, st));
    if(out_samples != nullptr) {
        PT_HIP(hipMemcpyAsync(out_samples, r0.pv_samples.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    PT_HIP(hipStreamSynchronize(st));
    return PT_OK;
}

} // extern "C"

// ---- temporal denoising of a sequence (pt_denoise.hip: pt_temporal_run) ----------------------------------------------------------------

// One sequence's history and scratch, all on `device` and owned by the handle (no shared workspace: two sequences may interleave).
struct pt_temporal {
    int device = 0;
    int32_t width = 0, height = 0;
    PtTemporalParams params{};
    std::mutex mutex;
    DevBuf<float4> col[2], guide, col_hist, pos[2], nrm[2], in_rgba, in_features;
    DevBuf<float> var[2];
    DevBuf<float2> grad, moments[2];
    DevBuf<int32_t> len[2];
    DevBuf<uint32_t> cls[2];
    int cur = 0;
    bool has_prev = false;
    PtDevCamera prev{};       // the last push's camera (its basis: all the feature rays depend on) ...
    float prev_rows[3][3] = {}; // ... and its reprojection rows (PtReprojection)
    PtDevCamera pending{};        // the same of the push in flight, until temporal_commit
    float pending_rows[3][3] = {};
};

namespace {

// The basis of `c` (derive_camera), its reprojection rows (PtReprojection) and its pixel footprint for images `height` pixels high;
// PT_ERR_INVALID for a degenerate basis.
int temporal_camera(const pt_camera_params *c, int32_t height, PtDevCamera *cam, float rows[3][3], float *footprint) {
    const float scalars[] = {c->origin[0], c->origin[1], c->origin[2], c->look_at[0], c->look_at[1], c->look_at[2], c->up[0], c->up[1], c->up[2],
                             c->focal_length, c->height, c->aspect_ratio};
    for(float v : scalars) {
        if(!std::isfinite(v)) {
            return fail(PT_ERR_INVALID, "camera: non-finite parameter");
        }
    }
    *cam = derive_camera(c);
    const Vec3 f = ld(cam->forward), u = ld(cam->up), r = ld(cam->right);
    Vec3 row[3] = {cross(u, r), cross(r, f), cross(f, u)}; // the inverse of [f u r], times det
    const float det = dot(f, row[0]);
    if(!std::isfinite(det) || det == 0.0F) {
        return fail(PT_ERR_INVALID, "camera: degenerate basis (look_at = origin, a zero up, height, focal length or aspect ratio, or up along the view)");
    }
    for(int i = 0; i < 3; i++) {
        if(det < 0.0F) { // (a negative aspect ratio): the same ratios, and "in front" stays row[0] . d > 0
            row[i] = scale(row[i], -1.0F);
        }
        const float v[3] = {row[i].x, row[i].y, row[i].z};
        for(int k = 0; k < 3; k++) {
            if(!std::isfinite(v[k])) {
                return fail(PT_ERR_INVALID, "camera: degenerate basis");
            }
            rows[i][k] = v[k];
        }
    }
    *footprint = c->height / (c->focal_length * static_cast<float>(height));
    return PT_OK;
}

int temporal_check_params(const pt_temporal_params &p) {
    if(p.spatial.iterations < 0 || p.spatial.iterations > 10) {
        return fail(PT_ERR_INVALID, "iterations must be 0..10");
    }
    for(float sigma : {p.spatial.sigma_luminance, p.spatial.sigma_normal, p.spatial.sigma_depth, p.sigma_luminance_temporal, p.position_tolerance}) {
        if(!std::isfinite(sigma) || sigma < 0.0F) {
            return fail(PT_ERR_INVALID, "sigmas and position_tolerance must be finite and not negative");
        }
    }
    for(float a : {p.alpha_color, p.alpha_moments}) {
        if(!(a > 0.0F && a <= 1.0F)) {
            return fail(PT_ERR_INVALID, "alphas must be in (0, 1]");
        }
    }
    if(p.max_history < 1 || p.moments_min_history < 1) {
        return fail(PT_ERR_INVALID, "max_history and moments_min_history must be at least 1");
    }
    if(!std::isfinite(p.normal_min)) {
        return fail(PT_ERR_INVALID, "normal_min must be finite");
    }
    return PT_OK;
}

// Checks a push's arguments without touching the handle or a device.
int temporal_check_push(const pt_temporal *t, const void *rgba, const void *features, const pt_camera_params *camera, const void *out) {
    if(t == nullptr || rgba == nullptr || features == nullptr || camera == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    PtDevCamera cam{};
    float rows[3][3];
    float footprint = 0.0F;
    return temporal_camera(camera, 1, &cam, rows, &footprint);
}

// Enqueues one push on `st` (handle mutex held by the caller).  The launch rewrites the colour history, so the handle has no usable history
// until the caller, once every copy of the push's outputs has succeeded, commits the push with temporal_commit; a failure in between leaves
// it with none (its next push starts afresh) rather than pairing this push's camera with the last push's buffers.
int temporal_push(pt_temporal *t, hipStream_t st, const float4 *rgba, const float4 *features, const pt_camera_params *camera, float4 *out) {
    PtReprojection rp{};
    PtDevCamera cam{};
    float rows[3][3];
    int rc = temporal_camera(camera, t->height, &cam, rows, &rp.footprint);
    if(rc != PT_OK) {
        return rc;
    }
    if(!t->has_prev) {
        rp.mode = PT_REPROJECT_NONE;
    }
    else if(std::memcmp(cam.origin, t->prev.origin, sizeof cam.origin) == 0 && std::memcmp(cam.forward, t->prev.forward, sizeof cam.forward) == 0 &&
            std::memcmp(cam.up, t->prev.up, sizeof cam.up) == 0 && std::memcmp(cam.right, t->prev.right, sizeof cam.right) == 0) {
        rp.mode = PT_REPROJECT_IDENTICAL;
    }
    else { // into the previous camera
        rp.mode = PT_REPROJECT_CAMERA;
        std::memcpy(rp.origin, t->prev.origin, sizeof rp.origin);
        std::memcpy(rp.row, t->prev_rows, sizeof rp.row);
    }
    PtDenoiseScratch s{};
    s.col[0] = t->col[0].ptr;
    s.col[1] = t->col[1].ptr;
    s.var[0] = t->var[0].ptr;
    s.var[1] = t->var[1].ptr;
    s.guide = t->guide.ptr;
    s.grad = t->grad.ptr;
    PtTemporalState state{};
    state.col_hist = t->col_hist.ptr;
    for(int i = 0; i < 2; i++) {
        state.moments[i] = t->moments[i].ptr;
        state.len[i] = t->len[i].ptr;
        state.pos[i] = t->pos[i].ptr;
        state.nrm[i] = t->nrm[i].ptr;
        state.cls[i] = t->cls[i].ptr;
    }
    state.cur = t->cur;
    t->has_prev = false;
    t->pending = cam;
    std::memcpy(t->pending_rows, rows, sizeof rows);
    PT_HIP(pt_temporal_run(st, rgba, features, t->width, t->height, t->params, rp, s, state, out));
    return PT_OK;
}

// The push enqueued by temporal_push has completed and its outputs were read: it becomes the history of the next push.
void temporal_commit(pt_temporal *t) {
    t->prev = t->pending;
    std::memcpy(t->prev_rows, t->pending_rows, sizeof t->prev_rows);
    t->has_prev = true;
    t->cur ^= 1;
}

} // namespace

extern "C" {

int pt_temporal_params_default(pt_temporal_params *out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    pt_denoise_params_default(&out->spatial);
    out->alpha_color = 0.2F;
    out->alpha_moments = 0.2F;
    out->max_history = 32;
    out->moments_min_history = 4;
    out->sigma_luminance_temporal = 4.0F;
    out->normal_min = 0.9F;
    out->position_tolerance = 2.0F;
    return PT_OK;
}

int pt_temporal_create(int device, int32_t width, int32_t height, const pt_temporal_params *params, pt_temporal **out) {
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    *out = nullptr;
    if(width <= 0 || height <= 0) {
        return fail(PT_ERR_INVALID, "image size must be positive");
    }
    if(static_cast<long long>(width) * height > 0x0fffffffLL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    pt_temporal_params p{};
    pt_temporal_params_default(&p);
    if(params != nullptr) {
        p = *params;
    }
    int rc = temporal_check_params(p);
    if(rc != PT_OK) {
        return rc;
    }
    const int n_dev = device_count_quiet();
    if(n_dev <= 0) {
        return fail(PT_ERR_NO_DEVICE, "no HIP device available; libpathtrace_hip has no CPU path");
    }
    if(device < 0 || device >= n_dev) {
        return fail(PT_ERR_NO_DEVICE, "device index out of range");
    }
    std::unique_ptr<pt_temporal> t(new pt_temporal());
    t->device = device;
    t->width = width;
    t->height = height;
    t->params = PtTemporalParams{PtDenoiseParams{p.spatial.iterations, p.spatial.sigma_luminance, p.spatial.sigma_normal, p.spatial.sigma_depth},
                                 p.alpha_color, p.alpha_moments, p.max_history, p.moments_min_history, p.sigma_luminance_temporal, p.normal_min,
                                 p.position_tolerance};
    const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
    PT_HIP(hipSetDevice(device));
    PT_HIP(t->guide.ensure(n));
    PT_HIP(t->col_hist.ensure(n));
    PT_HIP(t->grad.ensure(n));
    for(int i = 0; i < 2; i++) {
        PT_HIP(t->col[i].ensure(n));
        PT_HIP(t->var[i].ensure(n));
        PT_HIP(t->moments[i].ensure(n));
        PT_HIP(t->len[i].ensure(n));
        PT_HIP(t->pos[i].ensure(n));
        PT_HIP(t->nrm[i].ensure(n));
        PT_HIP(t->cls[i].ensure(n));
    }
    *out = t.release();
    return PT_OK;
}

int pt_temporal_denoise(pt_temporal *t, const float *rgba, const float *features, const pt_camera_params *camera, float *out_rgba, int32_t *out_history) {
    int rc = temporal_check_push(t, rgba, features, camera, out_rgba);
    if(rc != PT_OK) {
        return rc;
    }
    std::lock_guard<std::mutex> lock(t->mutex);
    const size_t n = static_cast<size_t>(t->width) * static_cast<size_t>(t->height);
    PT_HIP(hipSetDevice(t->device));
    PT_HIP(t->in_rgba.ensure(n));
    PT_HIP(t->in_features.ensure(3 * n));
    PT_HIP(hipMemcpy(t->in_rgba.ptr, rgba, n * sizeof(float4), hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(t->in_features.ptr, features, 3 * n * sizeof(float4), hipMemcpyHostToDevice));
    // in place, as pt_denoise
    rc = temporal_push(t, nullptr, t->in_rgba.ptr, t->in_features.ptr, camera, t->in_rgba.ptr);
    if(rc != PT_OK) {
        return rc;
    }
    PT_HIP(hipMemcpy(out_rgba, t->in_rgba.ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
    if(out_history != nullptr) {
        PT_HIP(hipMemcpy(out_history, t->len[t->cur].ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    temporal_commit(t);
    return PT_OK;
}

int pt_temporal_denoise_device(pt_temporal *t, const float *d_rgba, const float *d_features, const pt_camera_params *camera, float *d_out_rgba,
                               int32_t *d_out_history, void *stream) {
    int rc = temporal_check_push(t, d_rgba, d_features, camera, d_out_rgba);
    if(rc != PT_OK) {
        return rc;
    }
    std::lock_guard<std::mutex> lock(t->mutex);
    const size_t n = static_cast<size_t>(t->width) * static_cast<size_t>(t->height);
    PT_HIP(hipSetDevice(t->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = temporal_push(t, st, reinterpret_cast<const float4 *>(d_rgba), reinterpret_cast<const float4 *>(d_features), camera, reinterpret_cast<float4 *>(d_out_rgba));
    if(rc != PT_OK) {
        return rc;
    }
    if(d_out_history != nullptr) {
        PT_HIP(hipMemcpyAsync(d_out_history, t->len[t->cur].ptr, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    }
    PT_HIP(hipStreamSynchronize(st));
    temporal_commit(t);
    return PT_OK;
}

int pt_temporal_reset(pt_temporal *t) {
    if(t == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(t->mutex);
    t->has_prev = false;
    return PT_OK;
}

int pt_temporal_destroy(pt_temporal *t) {
    if(t == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    (void)hipSetDevice(t->device);
    delete t;
    return PT_OK;
}

} // extern "C"
