// pt_kernels.h -- launch interface between the host side of libpathtrace_hip.so (pt_render.cpp, pt_frames.cpp, pt_frame_maps.cpp,
// pt_image.cpp) and the kernels of pt_path.hip, pt_walks.hip and pt_frame.hip.
#ifndef PT_KERNELS_H
#define PT_KERNELS_H

#include <hip/hip_runtime.h>

#include "pt_types.h"

// flag bits of a stream slot
#define PT_F_DONE 1u      /* the slot will never hold a stream again */
#define PT_F_IN_FLIGHT 2u /* a path is in flight (otherwise the next invocation starts a sample) */
#define PT_F_HAS_EXT 4u   /* an extension (camera/bounce) ray was traced for it */
#define PT_F_COLLECTED 8u /* sample_collected (worker.cpp:37) */
#define PT_F_PIXEL 16u    /* the estimator of the current pixel is initialised */
#define PT_F_SAFE 64u     /* the estimator cannot stop at the sample in flight and another sample of the pixel follows (see pt_path.hip) */
#define PT_F_OVERLAP 32u  /* the next sample's camera ray is already in flight while the previous sample waits for its last shadow rays */

#define PT_DEST_SHADOW 0x80000000u
#define PT_DEST_NULL 0xffffffffu /* hole in the queue: reserved but not used */

// ---- the persistent path kernel (pt_path.hip) ---------------------------------------------------------------------------------------
// One launch renders a whole set of streams.  Every wavefront of the grid is an independent renderer: it owns `rows` x 64 stream SLOTS,
// a ray queue of its own and its share of the per-slot path state, and alternates between shading the slots whose rays have come back
// and tracing the rays that produced -- without ever synchronising with another wavefront.  A slot that has finished its stream pulls
// the next one from a global counter.

// Small tables the shading pass reads per lane live in LDS when they have at most PT_LDS_TABLE_MAX entries: the emitters' CDF (4 B),
// sampling records (64 B) and shading records (96 B: the vertex normals of an emissive triangle), and the materials (64 B).
#define PT_LDS_TABLE_MAX 16
#define PT_LDS_TABLE_BYTES (PT_LDS_TABLE_MAX * (4 + 64 + 96 + 64))
#define PT_WALK_SAVE_WORDS 13
#define PT_MAX_ROWS 8      /* rows of 64 slots per wavefront */
#define PT_F_STREAM 128u   /* the slot holds a stream (flag bit, next to PT_F_*) */

// Path state of the slots: PT_SLOT_PLANES planes of 16-byte records, plane k of slot p at state[k * total + p].  Slot index = (global wave
// index * rows + row) * 64 + lane, so that every access of a shading pass over one row is one coalesced run of 64 records: one
// dwordx4 load or store per plane, addressed as the scalar `state` plus a 32-bit byte offset (the host keeps the whole state below 4 GiB).
#define PT_PLANE_RAY_O 0    /* current ray origin xyz; w = contribution_unweighted (worker.cpp:38) */
#define PT_PLANE_RAY_D 1    /* current ray direction xyz; w = bits of path_length (worker.cpp:43) */
#define PT_PLANE_PD 2       /* (sample_divisor, sample_bounce_pd) as two doubles (worker.cpp:39-40) */
#define PT_PLANE_ENGINE 3   /* xorshift state of the stream's engine (x, y), index of the current pixel inside the rectangle (z), stream index (w) */
#define PT_PLANE_SPECTRUM 4 /* sample_spectrum (worker.cpp:41) */
#define PT_PLANE_OUT 5      /* out_spectrum (worker.cpp:42) */
#define PT_PLANE_RECT 6     /* the stream's WorkItem rectangle (written when the slot takes the stream) */
#define PT_SLOT_PLANES 7
struct PtSlots {
    uint32_t total;        // slots of the whole grid (stride of the planes and of the `nee` planes)
    float4 *state;         // [PT_SLOT_PLANES][total]
    float4 *nee;           // [light samples per vertex][total] weighed_spectrum of the pending shadow rays (worker.cpp:97)
    uint32_t *nee_mask;    // which of them wait for their shadow ray (or needed none): bit per light sample
    uint32_t *cost;        // wave steps the stream's rays spent in traversal so far (only when PtStreams::cost is wanted)
    PtEstimator *est;      // per-pixel estimator (worker.cpp:172-192)
    PtCandidate *cand;     // [total][PT_MAX_CANDIDATES]
};

// The streams of one render call.  Either explicit (rect + engine state per stream: processItem calls) or the pixels of a tile list, each
// its own 1x1 stream seeded from (base_seed, x, y) (processJob): then rect and rng are null and stream i is pixel i of the tiles laid end
// to end.
struct PtStreams {
    uint32_t n;
    const int4 *rect;            // [n] or null
    uint64_t *rng;               // [n] engine state in, engine state out; or null
    const int4 *tiles;           // [n_tiles] x, y, w, h
    const uint32_t *tile_offset; // [n_tiles] first stream of each tile
    uint32_t n_tiles;
    uint64_t base_seed;
    uint32_t first_total;        // streams 0 .. first_total-1 belong to the wavefronts' slots from the start (wavefront * slots_per_wave + slot)
    uint32_t first_lanes;        // streams per piece of the first round (64 = a row of slots; 32, 16: parts of a row)
    uint32_t first_shift;        // sideways steps per piece
    uint32_t n_waves, first_spread; // first_spread: row r of wavefront w starts on the 64-stream chunk r * n_waves + w ...
    uint32_t tiles_per_row, chunks_per_tile; // ... moved sideways by r * tiles_per_row / 4 tiles in a regular tile grid (0 = no grid)
    uint32_t *next;              // global pull counter (alone in its cache line)
    uint32_t *tile_left;         // [n_tiles] pixels of the tile not yet finished, or null: no progress reporting
    uint32_t *tiles_done;        // HOST-visible count of finished tiles (pinned memory), or null
    uint32_t *cost;              // [n] out, or null: traversal steps of the wavefront that passed while a ray of the stream was walking (summed over its rays)
    const uint32_t *place;       // [n_waves * slots per wave] or null: the stream that starts in every slot (0xffffffff: none) instead of the arithmetic first round
    const uint32_t *cancel;      // HOST-written stop request (pinned, fine-grained), or null: never stop.  Read once per shading pass; once it
                                 // is non-zero the wavefront takes no more streams and drops every stream that would start another sample
    // A resumable frame (pt_frame_render; all null otherwise).  With `todo`, stream i of the launch is stream todo[i].x of the frame (the
    // index into the tile table), and todo[i].y names its park record in park_in, or PT_NO_PARK: it starts afresh from its seed.
    const uint2 *todo;           // [n] or null
    const PtParkRecord *park_in; // the records todo names
    PtParkRecord *park_out;      // [park_cap]: a stream dropped by a stop request with samples taken parks here (one record per slot at most)
    uint32_t *park_count;        // records written to park_out
    uint32_t park_cap;
    uint32_t *status;            // [streams of the frame] or null: PT_STREAM_* of every stream this launch finished or parked
    // A pass of a progressive frame (pt_frame_set_progressive; 0 = off, and every test of it is wave-uniform): a stream whose pixel has taken
    // yield_at samples parks at that sample boundary as after a stop request -- exactly yield_at, since PtDevOptions::overlap_bound keeps the
    // sample that reaches it from being overlapped with its successor -- and frees its slot, which takes the next stream: the pool stays open.
    // A launch with yield_at may therefore park one stream per entry of its work list (park_cap = n), and counts them in streams_abandoned.
    int32_t yield_at;
    // A batch of views (pt_render_views): n_views > 1 frames of opt.image_height rows stacked into one tall image, view v = rows
    // [v * H, (v + 1) * H).  A pixel's view is its row / H; it is seeded from (view_seed[view], x, row - view * H) and its camera ray is
    // made by views[view] at that local row.  n_views <= 1: base_seed and the launch's camera, as every other entry point.
    uint32_t n_views, view_height; // view_height = opt.image_height (H)
    const PtViewCamera *views;   // [n_views] or null
    const uint64_t *view_seed;   // [n_views] or null
};

// Ray queues, one private ring per wavefront: entries [wave * cap, (wave + 1) * cap)
struct PtLocalQueue {
    float4 *ray_o;   // origin xyz, w = shadow threshold |to_light| - epsilon (worker.cpp:86) or unused
    float4 *ray_d;   // direction xyz, w = bits destination: bit 31 = shadow ray, bits 16..19 = light sample, bits 0..15 = slot of the wave
    uint32_t cap;    // rows * 64 * rays per slot
};

struct PtPathConfig {
    int grid;             // workgroups of 256 threads
    int rows;             // rows of 64 slots per wavefront (<= PT_MAX_ROWS)
    int slots_per_wave;   // slots a wavefront really uses (<= rows * 64; fewer for small jobs)
    int wide;             // more than 8 light samples per path vertex: the slots use the 64-bit word (pt_path.hip, SlotWord)
    int stack_lds;        // traversal stack entries per lane kept in LDS
    uint32_t spill_depth; // further entries per lane in HBM
    uint2 *spill;
    uint32_t *walk_save;  // [PT_WALK_SAVE_WORDS][grid * 256]: where a lane parks its walk during a shading pass
    size_t lds_bytes;
    int in_lds;           // whole tree + triangle records staged in LDS (small scenes)
    int refill_idle;      // idle lanes that make a wavefront refill from its queue (or shade when the queue is empty)
    int min_ready;        // slots that must be ready before a wavefront with walks in progress stops tracing to shade ...
    int ready_shift;      // ... or (slots that still hold or may get a stream) >> ready_shift, if that is less: a wavefront whose last streams are running shades them as they come
    int pass_q_low;       // a pass may also start while the ring still holds rays, if it holds at most this many ...
    int early_ready;      // ... and this many slots are ready (0 = never: a pass waits for the ring to run empty)
    int compact_passes;   // a pass whose ready slots fit fewer chunks of 64 than they occupy rows runs over a list of them (pt_path.hip)
    int debug_lanes;      // diagnostic: lanes of a wavefront that take rays (64)
    int burst_steps;      // traversal steps between two looks at the queue
    int first_lanes;      // slots per piece of the first round of streams (slots_per_wave is a multiple of it)
    int leaf_min;         // lanes that must stand on a leaf before the leaf code runs (while other lanes still have nodes to visit)
    unsigned long long *wave_counters; // [grid * 4 waves][8] node visits, leaf tests, rays, shadow rays, wave steps, shading passes, samples, vertices
};

// Everything the path kernel is told, in DEVICE memory: the kernel takes one pointer and reads what it needs where it needs it -- the
// traversal loop a handful of values once, a shading pass the rest each time it runs -- instead of holding ~100 scalar registers of
// kernel arguments live through the traversal loop (they do not fit: the compiler parked them in vector-register lanes there).
struct PtPathArgs {
    PtDevScene sc;
    PtDevCamera cam;
    PtDevOptions opt;
    PtSlots S;
    PtStreams T;
    PtLocalQueue Q;
    int rows, slots_per_wave, refill_idle, min_ready, burst_steps, leaf_min, ready_shift, pass_q_low, early_ready, compact_passes, debug_lanes;
    uint2 *spill;
    uint32_t spill_depth;
    uint32_t save_stride;
    uint32_t *walk_save;
    float4 *image;
    PtDevCounters *counters;
    unsigned long long *wave_counters;
};

// fills *host_args (which must stay valid until the launch has been issued), copies it to d_args on `stream` and launches
void pt_launch_path(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, const PtDevOptions &options, PtSlots slots, PtStreams streams,
                    PtLocalQueue queue, const PtPathConfig &cfg, float4 *image, PtDevCounters *counters, PtPathArgs *host_args, PtPathArgs *d_args);
// the work list of a resumable frame's next launch (pt_frame.hip): the streams of `todo` that `status` does not call finished, in two
// parts, each in the order of `todo`, and what the list holds in result[PT_COMPACT_*].  block_counts: [3 * ceil(n / 1024)].  Returns 0, or
// 1 when a launch failed.
// target <= 0, a plain frame: parked streams first, then untouched ones; park_in, park_out and park_count are not used.
// target > 0, a progressive frame's pass: streams below `target` samples first, then those at or above it; every stream keeps its record,
// and those the launch never claimed are copied from park_in (the launch's input records) into park_out behind the park_count records the
// launch wrote (park_cap: room for every entry, so that PT_COMPACT_NO_ROOM stays 0).
// noise.target > 0 (a progressive frame with a noise target, pt_frame_set_noise_target): a third part behind those two, the HELD streams:
// those with a record whose pixel_error (pt_noise.h) is at or below noise.target.  resort != 0: nothing was launched (every status is
// untouched) and the list is only split again -- no record moves, park_in stays the frame's records, park_out is not used.
enum PtCompactWord {
    PT_COMPACT_FIRST = 0,        // streams of the first part
    PT_COMPACT_SECOND,           // ... and of the second
    PT_COMPACT_LOST,             // plain frame: untouched streams whose earlier record went unused (such a stream starts afresh)
    PT_COMPACT_CARRIED,          // samples the streams of the list carry
    PT_COMPACT_WITH_CANDIDATES,  // streams with closed candidates
    PT_COMPACT_MIN_INVERTED,     // 0xffffffff - the least sample count of an unfinished pixel (a minimum over a word that starts at zero)
    PT_COMPACT_MAX,              // the greatest
    PT_COMPACT_WITH_RECORD,      // streams that have a record
    PT_COMPACT_WRITTEN,          // records the launch wrote
    PT_COMPACT_NO_ROOM,          // samples of records that found no room in park_out
    PT_COMPACT_HELD,             // streams of the third part
    PT_COMPACT_WORDS = 16
};
// what the compaction makes of one entry: the part of the list it goes to, and where the stream's record is
enum PtEntryClass : uint32_t { PT_ENTRY_FINISHED = 0, PT_ENTRY_FIRST = 1, PT_ENTRY_SECOND = 2, PT_ENTRY_HELD = 3 };
enum PtEntryRecord : uint32_t { PT_RECORD_NONE = 0, PT_RECORD_WRITTEN = 1 /* park_out, by the launch */, PT_RECORD_UNCLAIMED = 2 /* park_in */ };
struct PtNoiseRule {
    PtDevOptions opt; // (its stats_sample_count: the samples of a batch mean)
    float target;     // 0 = none: nothing is held
    float floor;
};
int pt_launch_frame_compact(hipStream_t stream, const uint2 *todo, uint32_t n, uint32_t *status, const PtParkRecord *parked, uint2 *todo_out, uint32_t *block_counts,
                            unsigned long long *result, int32_t target, const PtParkRecord *park_in, PtParkRecord *park_out, uint32_t *park_count, uint32_t park_cap,
                            const PtNoiseRule &noise, int resort);
// The rating of a frame (pt_frame.hip; pt_frame_get_noise).  rate: out[i] = (pixel, bits of pixel_error) per entry of a replica's work list
// and the summary (zeroed first).  base: the map of replica 0's device, -1 where cover[p] != 0, else +inf.  scatter: n entries into the map.
enum PtNoiseWord {
    PT_NOISE_RATED = 0,
    PT_NOISE_UNRATED,
    PT_NOISE_HELD,      // rated, and error <= noise.target > 0
    PT_NOISE_MAX_BITS,  // the largest bit pattern of the error of a rated entry, as an unsigned word: the largest error, or a NaN if one rates NaN
    PT_NOISE_FIRST_BIN, // rated entries by pixel_error_bin: 64 bins
    PT_NOISE_SUMMARY_WORDS = PT_NOISE_FIRST_BIN + 64
};
int pt_launch_frame_rate(hipStream_t stream, const uint2 *todo, uint32_t n, const PtParkRecord *park, const int4 *tiles, const uint32_t *tile_offset, uint32_t n_tiles,
                         int32_t width, const PtNoiseRule &noise, uint2 *out, uint32_t *summary);
int pt_launch_frame_noise_base(hipStream_t stream, float *map, const uint8_t *cover, uint32_t n_pixels);
int pt_launch_frame_noise_scatter(hipStream_t stream, const uint2 *rated, uint32_t n, float *map);
// The variance map of a frame (pt_frame.hip; pt_frame_get_variance).  variance: out_var[i] = pixel_variance (pt_noise.h) per entry of a
// replica's work list, (0, 0, 0, 0) for an entry without a record, and out_at[i] its pixel.  scatter: n entries into the map of replica 0's
// device, which starts as zeros.  Each returns 0, or 1 when the launch failed.
int pt_launch_frame_variance(hipStream_t stream, const uint2 *todo, uint32_t n, const PtParkRecord *park, const int4 *tiles, const uint32_t *tile_offset,
                             uint32_t n_tiles, int32_t width, const PtDevOptions &opt, float4 *out_var, int32_t *out_at);
int pt_launch_frame_variance_scatter(hipStream_t stream, const float4 *var, const int32_t *at, uint32_t n, float4 *map);
// The preview of a frame (pt_frame.hip; pt_frame_preview).  gather: one compact entry per entry of a replica's work list todo[0 .. n), those
// that name a record (the first n_parked of a plain frame) parked in `park` -- out_rgba the running mean (0 for an untouched stream), out_at (y * width + x, samples taken).  base: the
// view of replica 0's device, which holds the caller's image: samples -1 where cover[p] != 0, else a hole (0, 0, 0, 0) with 0 samples.
// scatter: the n entries into the view.  Each returns 0, or 1 when the launch failed.
int pt_launch_frame_gather(hipStream_t stream, const uint2 *todo, uint32_t n, uint32_t n_parked, const PtParkRecord *park, const int4 *tiles,
                           const uint32_t *tile_offset, uint32_t n_tiles, int32_t width, float4 *out_rgba, int2 *out_at);
int pt_launch_frame_preview_base(hipStream_t stream, float4 *view, int32_t *samples, const uint8_t *cover, uint32_t n_pixels);
int pt_launch_frame_scatter(hipStream_t stream, const float4 *rgba, const int2 *at, uint32_t n, float4 *view, int32_t *samples);
int pt_path_blocks_per_cu(const PtPathConfig &cfg); // resident workgroups per CU of the instantiation cfg selects (wide, in_lds, stack_lds) with cfg.lds_bytes
size_t pt_path_lds_bytes(int wide, int rows, int stack_lds, uint32_t n_lds_pairs, uint32_t n_lds_leaf_records); // leaf records: triangles + 1 spare + spheres, 0 = scene not in LDS
int pt_path_stack_lds(int in_lds, size_t lds_bytes_with_default_window); // entries of the stack window: 8, or 4 for a scene in LDS that would not leave room for four workgroups per CU
// ---- one walk per lane (pt_walks.hip) -----------------------------------------------------------------------------------------------
// diagnostic (tools/replay_probe.py): the traversal alone over the rays a render left in its rings; returns the resident workgroups per CU
int pt_launch_replay(hipStream_t stream, const PtDevScene &scene, const PtLocalQueue &Q, uint32_t n_logs, uint32_t parts, int waves_per_simd, const PtPathConfig &cfg,
                     uint2 *spill, unsigned long long *out);
// Scene::getIntersection for n rays (6 floats each): out[i] = (bits t, ref)
void pt_launch_closest(hipStream_t stream, const PtDevScene &scene, const float *rays6, uint32_t n, uint2 *out, const PtPathConfig &cfg);
// Features of a width x height frame for the denoiser (pt_walks.hip): out[3 * pixel + k], k = albedo + coverage, normal + t, position +
// emission luminance.  views == nullptr: the frame of `camera`, which travels in the kernel's arguments and must have no aperture sampler.
// Otherwise n_views frames in one launch: out[3 * ((v * height + y) * width + x) + k] is what the single frame gives pixel (x, y) with
// views[v].cam (a DEVICE table whose cameras have no aperture; `camera` is not read).  follow == nullptr: first hits (pt_feature_kernel).
// Otherwise rays that go on through glass and mirrors for at most max_bounces bounces (pt_follow_kernel; include/pt_features.h; 0: the
// bits of the first-hit pass), epsilon being pt_options'.  The walk and its instantiation are pt_launch_closest's; cfg.spill holds one
// walk per pixel of every view.
struct PtFollow {
    int32_t max_bounces;
    float epsilon;
};
void pt_launch_features(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, const PtViewCamera *views, int32_t n_views, int32_t width, int32_t height,
                        float4 *out, const PtPathConfig &cfg, const PtFollow *follow);
// The first-hit features of ONE frame and its motion in one launch (pt_motion_kernel; include/pt_motion.h): `out` as
// pt_launch_features gives it without views and without follow, bit for bit, and motion[2 * pixel + k], k = previous position + fraction
// moved, previous normal + fraction without a previous position.  `instances` (device memory) holds the n_instances mesh instances that
// have objects, by ascending first object; their ranges are disjoint.  n_instances == 0: nothing moved, and `instances` is not read.
struct alignas(16) PtMotionInstance {
    uint32_t first, count; // the instance's objects: first .. first + count - 1, count > 0
    uint32_t kind;         // PT_MOTION_STATIC | PT_MOTION_MOVED | PT_MOTION_NONE
    uint32_t pad;
    float back[12];        // previous position = back * (position, 1): 3 rows of 4
    float normal[12];      // previous normal direction = normal * normal: 3 rows of 3, each padded to 4
};
void pt_launch_features_motion(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, int32_t width, int32_t height, float4 *out, float4 *motion,
                               const PtMotionInstance *instances, uint32_t n_instances, const PtPathConfig &cfg);
// The same for a scene marked by pt_scene_motion_mark whose meshes were deformed since (pt_motion_shapes_kernel;
// include/pt_motion_shapes.h): an instance of kind PT_MOTION_DEFORMED (3) finds the face its hit triangle came from
// (face_of[object - first_object]: one word per instance triangle), that face's three vertices as they were at the mark, and the matrix
// the instance had then.  The other kinds are pt_motion_kernel's, operation for operation.
struct alignas(16) PtShapeMotionInstance {
    uint32_t first, count; // as PtMotionInstance's
    uint32_t kind;         // PT_MOTION_STATIC | PT_MOTION_MOVED | PT_MOTION_NONE | PT_MOTION_DEFORMED
    uint32_t face_first;   // the scene-wide number of the instance's face 0
    float back[12];
    float normal[12];
    const int32_t *faces;  // device, [n_faces][3]: the instance's mesh
    const float *marked;   // device, [n_vertices][3]: the mesh's vertices at the mark
    float m[16];           // rows of the instance's matrix at the mark
};
void pt_launch_features_motion_shapes(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, int32_t width, int32_t height, float4 *out, float4 *motion,
                                      const PtShapeMotionInstance *instances, uint32_t n_instances, const uint32_t *face_of, uint32_t first_object, const PtPathConfig &cfg);
// face_of[rank[f]] = face_base_scene + f for every face f < n_faces of a chunk with flag[f] != 0 and rank[f] < room (pt_face_table_kernel,
// pt_motion_shapes_kernels.h): `flag` and `rank` are what pt_mesh_batch_chunk left in its scratch, face_of points at the chunk's first triangle
hipError_t pt_face_table_launch(hipStream_t stream, const uint32_t *flag, const uint32_t *rank, uint32_t n_faces, uint64_t room, uint32_t *face_of, uint32_t face_base_scene);
// Scene queries (pt_query_kernels.h; include/pt_query.h): out[4 * i + k] is the k-th 16 bytes of query i's pt_hit.  The walk
// and its instantiation are pt_launch_closest's; cfg.spill holds one walk per query.  `tables`: the instances that have objects by
// ascending first object (device memory; n_inst == 0: none is read), and the scene's face table (null: there is none) with the object
// its entry 0 belongs to.
struct alignas(16) PtQueryInstance {
    uint32_t first, count; // the instance's objects: first .. first + count - 1, count > 0
    uint32_t face_first;   // the scene-wide number of the instance's face 0
    uint32_t n_faces;      // faces of its mesh: count == n_faces means every face survived
    uint32_t instance;     // its index in the scene's instance list
    uint32_t pad[3];
};
struct PtQueryTables {
    const PtQueryInstance *inst;
    uint32_t n_inst;
    uint32_t first_object;
    const uint32_t *face_of;
};
void pt_launch_query_rays(hipStream_t stream, const PtDevScene &scene, const float *rays6, uint32_t n, float4 *out, const PtQueryTables &tables, const PtPathConfig &cfg);
// the rays through the centres of the pixels xy[n][2] of camera's width x height frame (no aperture), or with xy == nullptr of all n = width * height pixels in row order
void pt_launch_query_pixels(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, int32_t width, int32_t height, const int32_t *xy, uint32_t n, float4 *out,
                            const PtQueryTables &tables, const PtPathConfig &cfg);
// out[i] = 1 iff the closest hit of segment i (origin, direction, t_max: 7 floats) has 0 <= t < t_max: the shadow walk, ended at the first such leaf
void pt_launch_occluded(hipStream_t stream, const PtDevScene &scene, const float *seg7, uint32_t n, uint8_t *out, const PtPathConfig &cfg);
// Light gathered at points (pt_gather_kernels.h; include/pt_gather.h): the samples of the points first .. first + n_points - 1
// of points6 (position, normal; `miss`, if not null, marks the points that are not there) into the chunk's workspace -- plane[n_points *
// samples] for kinds 1 and 2, bits[ceil(n_points * samples / 64)] for kind 0 --, then their records out[2 * point], out[2 * point + 1] by the
// ordered reduce.  n_points * samples <= 0x7fffffff; cfg.spill holds one walk per pair of the chunk.
void pt_launch_gather(hipStream_t stream, const PtDevScene &scene, int kind, const float *points6, const uint8_t *miss, uint32_t first, uint32_t n_points, uint32_t samples,
                      float epsilon, float distance, uint64_t base_seed, float4 *plane, unsigned long long *bits, float4 *out, const PtPathConfig &cfg);
// the points of a frame's first hits (pt_query_frame's rays; the normal turned against the ray) and which pixels have none; cfg.spill holds one walk per pixel
void pt_launch_gather_frame_points(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, int32_t width, int32_t height, float *points6, uint8_t *miss,
                                   const PtPathConfig &cfg);
// the corners of the triangles first_tri .. first_tri + n_tris - 1 with their normals: 3 points per triangle
void pt_launch_gather_corner_points(hipStream_t stream, const float *pos, const float4 *shade, uint32_t first_tri, uint32_t n_tris, float *points6);
// Light probes (pt_light_probe_kernels.h; include/pt_light_probes.h).  A grid as the kernels take it: pt_light_probe_grid's fields
struct PtLightProbeGrid {
    float origin[3];
    float step[3];
    uint32_t count[3];
};
// The samples of the probes first .. first + n_probes - 1 -- at positions[3 * probe], or, with positions == null, at the grid's nodes -- into
// the chunk's workspace plane[2 * n_probes * samples] (radiance; direction and flags), then their 128-byte records out[8 * probe ..] by the
// projection, one wavefront per probe.  n_probes * samples <= 0x7fffffff; cfg.spill holds one walk per pair of the chunk.
void pt_launch_light_probes(hipStream_t stream, const PtDevScene &scene, const float *positions, const PtLightProbeGrid &grid, uint32_t first, uint32_t n_probes, uint32_t samples,
                            float epsilon, uint64_t base_seed, float4 *plane, float4 *out, const PtPathConfig &cfg);
// out[i] = the blend of the grid's records (8 float4 each) around point i (position, normal), evaluated towards its normal, and the sum of the weights
void pt_launch_light_probe_shade(hipStream_t stream, const PtLightProbeGrid &grid, const float4 *probes, float max_backfacing, const float *points6, uint32_t n, float4 *out);
// Radiance along free rays and captures (pt_radiance_kernels.h; include/pt_radiance.h).  A capture as the kernels take it:
// pt_capture_desc's fields, the model one of PT_CAPTURE_*
#define PT_CAPTURE_MODEL_EQUIRECT 0
#define PT_CAPTURE_MODEL_CUBE 1
#define PT_CAPTURE_MODEL_FISHEYE 2
#define PT_CAPTURE_MODEL_ORTHO 3
struct PtCaptureParams {
    int32_t model, width, height, jitter;
    float origin[3], right[3], up[3], forward[3];
    float fov;
    float extent[2];
};
// The samples of the rays (rays[6 * i], origin and direction) or, with rays == null, of the capture's pixels first .. first + n - 1 into the
// chunk's workspace plane[n * samples] (radiance and flags), then their 32-byte records out[2 * i ..] by the reduction, one wavefront
// each.  n * samples <= 0x7fffffff; cfg.spill holds one walk per pair of the chunk.
void pt_launch_radiance(hipStream_t stream, const PtDevScene &scene, const float *rays, const PtCaptureParams &capture, uint32_t first, uint32_t n, uint32_t samples, float epsilon,
                        uint64_t base_seed, float4 *plane, float4 *out, const PtPathConfig &cfg);
// Light-group passes (pt_light_pass_kernels.h; include/pt_light_passes.h).  The samples of pt_launch_radiance's rays or
// pixels into plane[n * samples] as there and into the pass accumulators passes[n_passes * n * samples] (pass-major), then the 16-byte pass
// records out_passes[(first + i) * n_passes + p] by a reduction of one wavefront each and, with out_total, the 32-byte records
// out_total[2 * (first + i) ..] by pt_launch_radiance's own reduction.  groups: the group of every material, then of every point light
// (scene.n_materials + scene.n_lights bytes); n_passes = groups * (split ? 3 : 1) <= 24; n * samples * n_passes <= 0x7fffffff.
void pt_launch_light_passes(hipStream_t stream, const PtDevScene &scene, const float *rays, const PtCaptureParams &capture, uint32_t first, uint32_t n, uint32_t samples, float epsilon,
                            uint64_t base_seed, const uint8_t *groups, uint32_t n_passes, uint32_t split, float4 *plane, float4 *passes, float4 *out_passes, float4 *out_total,
                            const PtPathConfig &cfg);
// out[i] = the mix of passes[i * n_passes ..] under gains[n_passes][3], one thread each; alpha = total[2 * i].w, or 0 without total
void pt_launch_light_pass_mix(hipStream_t stream, const float4 *passes, size_t n, uint32_t n_passes, const float *gains, const float4 *total, float4 *out);
// Nearest-surface queries (pt_nearest_kernels.h, pt_nearest.hip; include/pt_nearest.h).  A grid as the kernel takes it:
// pt_distance_grid's fields
struct PtDistanceGrid {
    float origin[3];
    float step[3];
    uint32_t count[3];
};
// out[4 * (first + i) + k], i < n: the k-th 16 bytes of the pt_nearest of query first + i of points4 (xyz, max_distance).  spill holds
// spill_depth entries for each of the launch's ((n + 255) / 256) * 256 lanes.  counts (diagnostic; null in the product's calls): the
// pair and the leaf records the launch fetched are added to counts[0] and counts[1].
void pt_launch_nearest_points(hipStream_t stream, const PtDevScene &scene, const float *points4, uint32_t first, uint32_t n, float4 *out, const PtQueryTables &tables, uint2 *spill,
                              uint32_t spill_depth, unsigned long long *counts);
// out_distance[first + i] and (out_object not null) out_object[first + i], i < n: distance and object of the query at cell first + i of
// the grid with max_distance; the spill area as above
void pt_launch_nearest_grid(hipStream_t stream, const PtDevScene &scene, const PtDistanceGrid &grid, float max_distance, uint32_t first, uint32_t n, float *out_distance,
                            int32_t *out_object, uint2 *spill, uint32_t spill_depth);
// diagnostic (tools/step_timing.py): stamped walks, `lanes_per_wave` rays per wavefront; out[ray] = (steps, cycles waiting for records, cycles in all, price of a stamp pair)
void pt_launch_steptime(hipStream_t stream, const PtDevScene &scene, const float *rays6, uint32_t n, uint32_t lanes_per_wave, uint4 *out, uint2 *spill, uint32_t spill_depth, int flags);


#endif
