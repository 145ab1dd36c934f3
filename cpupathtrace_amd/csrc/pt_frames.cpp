// pt_frames.cpp -- resumable frames of the C ABI (include/pt_hip.h): pt_frame_create*, pt_frame_render and its progressive passes, the
// preview of an unfinished frame (pt_frame_preview) and the frame's queries.
#include "pt_host.h"

#include <limits>

using namespace pth;

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
        uint32_t n_held = 0;                      // streams at the list's end that the noise target holds (0 without one)
        int32_t min_samples = 0, max_samples = 0; // samples taken, over the list's pixels
        bool ready = false; // the device tables exist
        bool in_order = true; // the work list is every stream of the replica in order (stream i at index i)
        int cur = 0, pcur = 0; // todo[cur] and park[pcur] are what the next launch reads
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
        // pt_frame_get_noise: the replica's rated work list and its summary; on replica 0 also the error map, which pixels the tiles of
        // the replicas that have rendered cover (and how many such replicas that is) and the other replicas' entries on their way in
        DevBuf<uint2> nz_rated, nz_stage;
        DevBuf<uint32_t> nz_summary;
        DevBuf<float> nz_map;
        DevBuf<uint8_t> nz_cover;
        size_t nz_cover_ready = 0;
        // pt_frame_get_variance: the replica's gathered variances and their pixels; on replica 0 also the map and the other replicas'
        // entries on their way in
        DevBuf<F4> vr_var, vr_stage_var, vr_map;
        DevBuf<int32_t> vr_at, vr_stage_at;
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
    // the noise target (pt_frame_set_noise_target): a progressive frame holds the streams rated at or below noise_target (0 = none);
    // target_reached: the last pt_frame_render found enough of them held, and nothing has changed since
    float noise_target = 0.0f, noise_floor = 1E-5f, noise_fraction = 1.0f;
    bool target_reached = false;
    double noise_rate_ms = 0.0; // device time of the rating kernels of the last pt_frame_get_noise, all replicas (tools/noise_probe.py)
    // device time of the gather kernels of the last variance map, all replicas, and of the filter of the last denoised preview
    // (tools/measured_probe.py)
    double variance_gather_ms = 0.0, preview_filter_ms = 0.0;
    // pt_frame_set_feature_params: the denoised previews take followed features (include/pt_features.h) with these parameters
    bool follow_features = false;
    pt_feature_params feature_params{};
    PtNoiseRule noise_rule(const PtDevOptions &opt, bool holding) const {
        PtNoiseRule rule;
        rule.opt = opt;
        rule.target = holding ? noise_target : 0.0f;
        rule.floor = noise_floor;
        return rule;
    }
    bool holding() const { return quantum > 0 && noise_target > 0.0f; }
    int status = PT_OK; // a failed frame returns this (and `error`) from every later call
    std::string error;
    mutable std::mutex mutex; // one call at a time
};

namespace {

// The device tables of a replica, made by its first launch: the tile table, the first stream of every tile and its pixel count, the
// status of every stream (all untouched) and the first work list (every stream, none parked).
int frame_prepare(pt_frame::Replica &r) {
    const TileTable table(r.tiles.data(), r.tiles.size());
    std::vector<uint2> todo(r.n_streams);
    for(uint32_t i = 0; i < r.n_streams; i++) {
        todo[i] = make_uint2(i, PT_NO_PARK);
    }
    PT_HIP(r.d_tiles.upload(table.rects));
    PT_HIP(r.d_offset.upload(table.offsets));
    PT_HIP(r.d_left.upload(table.left));
    PT_HIP(r.d_todo[0].upload(todo));
    PT_HIP(r.d_todo[1].ensure(r.n_streams));
    PT_HIP(r.d_status.ensure(r.n_streams));
    PT_HIP(hipMemset(r.d_status.ptr, 0, static_cast<size_t>(r.n_streams) * sizeof(uint32_t)));
    PT_HIP(r.d_blocks.ensure(3 * ((static_cast<size_t>(r.n_streams) + 1023) / 1024)));
    PT_HIP(r.d_park_count.ensure(1));
    PT_HIP(r.d_park[0].ensure(1));
    PT_HIP(r.d_result.ensure(16));
    r.ready = true;
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
    PT_TRY(derive_options(&f.options, &opt));
    const PtDevCamera cam = derive_camera(&f.camera);
    if(!r.ready) {
        if(f.n_views > 1) {
            PT_HIP(r.d_view_cams.upload(f.views.cams));
            PT_HIP(r.d_view_seeds.upload(f.views.seeds));
        }
        PT_TRY(frame_prepare(r));
    }
    const size_t pixels = static_cast<size_t>(f.options.image_width) * static_cast<size_t>(f.rows());
    PT_HIP(s->image.ensure(pixels));
    PT_TRY(copy_tile_rects(s, r.tiles, r.index, f.tile_done.data(), out_image, static_cast<size_t>(f.options.image_width), true));
    // park storage: one record per slot at most (a stop closes the pool, so a slot drops one stream at most), and never more than the streams left.
    // A progressive pass keeps the pool open and every stream of the list leaves a record, written by the launch or carried over: one per entry.
    // (the streams a noise target holds are the end of the list: the launch does not see them, the next list keeps them)
    const bool progressive = yield_at > 0;
    const uint32_t n_launch = r.n_todo - (progressive ? r.n_held : 0u);
    PtPathConfig cfg;
    PT_TRY(ensure_path_workspace(s, n_launch, &cfg));
    const int cur = r.cur, next = cur ^ 1, pcur = r.pcur, pnext = pcur ^ 1;
    const uint32_t cap = progressive ? r.n_todo : std::min<uint32_t>(r.n_todo, s->path_slots);
    if(progressive) {
        opt.overlap_bound = std::min(opt.max_sample_count, yield_at); // (the sample that reaches the target ends at a boundary of its own)
    }
    PT_HIP(r.d_park[pnext].ensure(cap));
    PT_HIP(hipMemsetAsync(r.d_park_count.ptr, 0, sizeof(uint32_t), s->stream));
    PtStreams T{};
    set_tile_streams(&T, n_launch, r.d_tiles.ptr, r.d_offset.ptr, r.tiles.size(), f.base_seed, f.n_views, f.options.image_height, r.d_view_cams.ptr, r.d_view_seeds.ptr);
    // The first round is spread over the work list.  The first launch's list is every stream in order, so it is spread over the tile grid
    // as pt_render_tiles spreads it (an uninterrupted frame is scheduled exactly like one); a later list is no tile grid.
    T.tiles_per_row = 0;
    T.chunks_per_tile = 0;
    if(r.in_order) {
        tile_grid(r.tiles.data(), r.tiles.size(), &T.tiles_per_row, &T.chunks_per_tile);
    }
    T.tile_left = r.d_left.ptr;
    T.todo = r.d_todo[cur].ptr;
    T.park_in = r.d_park[pcur].ptr;
    T.park_out = r.d_park[pnext].ptr;
    T.park_count = r.d_park_count.ptr;
    T.park_cap = cap;
    T.status = r.d_status.ptr;
    T.yield_at = progressive ? yield_at : 0;
    PT_TRY(run_path(s, cam, opt, T, reinterpret_cast<float4 *>(s->image.ptr), stats, progress, progress_user, stop));
    PT_TRY(copy_tile_rects(s, r.tiles, r.index, f.tile_done.data(), out_image, static_cast<size_t>(f.options.image_width), false));
    PT_TRY(finish_path(s, &out->tally));
    if(pt_launch_frame_compact(s->stream, r.d_todo[cur].ptr, r.n_todo, r.d_status.ptr, r.d_park[pnext].ptr, r.d_todo[next].ptr, r.d_blocks.ptr, r.d_result.ptr,
                               progressive ? yield_at : 0, r.d_park[pcur].ptr, r.d_park[pnext].ptr, r.d_park_count.ptr, cap, f.noise_rule(opt, f.holding()), 0) != 0) {
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
    // (res[10]: the streams the noise target holds, launched or not)
    if(t.finished + res[0] + res[1] + res[10] != r.n_todo || res[8] > t.abandoned || res[7] > cap || (!progressive && res[8] != res[0]) || res[9] != 0) {
        return fail(PT_ERR_HIP, "frame: " + std::to_string(t.finished) + " finished, " + std::to_string(res[0]) + " parked and " + std::to_string(res[1]) +
                                    " left of " + std::to_string(r.n_todo) + " streams (" + std::to_string(t.abandoned) + " dropped, " + std::to_string(res[10]) + " held)");
    }
    r.n_todo = static_cast<uint32_t>(res[0] + res[1] + res[10]);
    r.n_parked = static_cast<uint32_t>(res[7]);
    r.n_held = static_cast<uint32_t>(res[10]);
    r.in_order = r.n_todo == r.n_streams && (r.n_parked == 0 || r.n_parked == r.n_todo) && (!progressive || std::max({res[0], res[1], res[10]}) == r.n_todo); // (each part in order)
    r.samples_carried = res[3];
    r.with_candidates = res[4];
    r.n_at_target = progressive ? static_cast<uint32_t>(res[1]) : 0;
    r.min_samples = r.n_todo != 0 ? static_cast<int32_t>(0xffffffffULL - res[5]) : 0;
    r.max_samples = static_cast<int32_t>(res[6]);
    r.cur = next;
    r.pcur = pnext;
    out->parked = res[8];
    for(size_t k = 0; k < left.size(); k++) {
        f.tile_done[r.index[k]] = left[k] == 0 ? 1 : 0;
    }
    return PT_OK;
}

// A progressive frame with a noise target, before a pass to `yield_at` samples: the replica's list split again by that sample count and
// the target as they are now -- streams below the count, streams at it, held streams -- with nothing launched and no record moved.
int frame_resort(pt_frame &f, pt_frame::Replica &r, int32_t yield_at) {
    if(!r.ready || r.n_todo == 0) {
        r.n_held = 0; // (no records yet: nothing is rated)
        return PT_OK;
    }
    pt_scene *s = r.s;
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtDevOptions opt;
    PT_TRY(derive_options(&f.options, &opt));
    const int cur = r.cur, next = cur ^ 1;
    if(pt_launch_frame_compact(s->stream, r.d_todo[cur].ptr, r.n_todo, r.d_status.ptr, r.d_park[r.pcur].ptr, r.d_todo[next].ptr, r.d_blocks.ptr, r.d_result.ptr,
                               yield_at, r.d_park[r.pcur].ptr, nullptr, nullptr, 0, f.noise_rule(opt, true), 1) != 0) {
        PT_HIP(hipGetLastError());
        return fail(PT_ERR_HIP, "frame: work list kernel failed to launch");
    }
    unsigned long long res[16];
    PT_HIP(hipMemcpyAsync(res, r.d_result.ptr, sizeof(res), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    if(res[0] + res[1] + res[10] != r.n_todo) {
        return fail(PT_ERR_HIP, "frame: " + std::to_string(res[0] + res[1]) + " streams to do and " + std::to_string(res[10]) + " held of " + std::to_string(r.n_todo));
    }
    r.in_order = r.in_order && std::max({res[0], res[1], res[10]}) == r.n_todo;
    r.n_at_target = static_cast<uint32_t>(res[1]);
    r.n_held = static_cast<uint32_t>(res[10]);
    r.cur = next;
    return PT_OK;
}

// What one round of launches left of the frame
struct FrameRound {
    uint64_t left = 0, parked = 0, at_target = 0, held = 0; // streams still to do, parked by this round, at the target of a progressive pass, held by the noise target
};

// the work of all of a call's launches; the grid is the last launch's
void add_stats(pt_stats &o, const pt_stats &p) {
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

// One round of launches of pt_frame_render: every replica that has work makes one (yield_at > 0: a pass of a progressive frame up to that
// sample count), each on its own thread.  Adds what they did to ctl and stats (both may be null); a failure fails the frame for good.
int frame_round(pt_frame *f, float *out_image, pt_stats *stats, SharedProgress *shared, RenderStop *stop, pt_render_control *ctl, int32_t yield_at, FrameRound *round) {
    const size_t n_scenes = f->reps.size();
    std::vector<FrameLaunch> launched(n_scenes);
    std::vector<char> ran(n_scenes, 0);
    std::vector<pt_stats> pass_stats(stats != nullptr ? n_scenes : 0, pt_stats{});
    const int rc = for_each_replica(static_cast<int>(n_scenes), [&](int i) -> int {
        pt_frame::Replica &r = *f->reps[static_cast<size_t>(i)];
        if(r.n_todo - (yield_at > 0 ? r.n_held : 0u) == 0) {
            return PT_OK; // (nothing left, or every stream left is held)
        }
        ran[static_cast<size_t>(i)] = 1;
        return frame_launch(*f, r, out_image, stats != nullptr ? &pass_stats[static_cast<size_t>(i)] : nullptr, shared->callback(), shared, stop, &launched[static_cast<size_t>(i)], yield_at);
    });
    for(size_t i = 0; i < n_scenes; i++) {
        f->launches += ran[i];
    }
    if(rc != PT_OK) {
        f->status = rc;
        f->error = "frame failed: " + last_error();
        return fail(f->status, f->error);
    }
    f->tiles_done = static_cast<uint64_t>(std::count(f->tile_done.begin(), f->tile_done.end(), 1));
    *round = FrameRound();
    if(ctl != nullptr) {
        ctl->streams_abandoned = ctl->streams_unclaimed = 0; // (of the call's last launches)
    }
    for(size_t i = 0; i < n_scenes; i++) {
        const FrameLaunch &l = launched[i];
        round->left += f->reps[i]->n_todo;
        round->at_target += f->reps[i]->n_at_target;
        round->held += f->reps[i]->n_held;
        round->parked += l.parked;
        if(ctl != nullptr) {
            ctl->streams_finished += l.tally.finished;
            ctl->streams_abandoned += l.parked;
            ctl->streams_unclaimed += l.tally.unclaimed + (l.tally.abandoned - l.parked); // (dropped before their first sample: they start afresh)
        }
        if(stats != nullptr) {
            add_stats(stats[i], pass_stats[i]);
        }
    }
    return PT_OK;
}

std::string noise_reached_message(uint64_t held, uint64_t left) {
    return "frame stopped (noise target reached): " + std::to_string(held) + " streams held, " + std::to_string(left) + " streams left";
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
    PT_TRY(check_tiles(tiles, n_tiles, options->image_width, rows, &total, "frame"));
    PtDevOptions opt;
    PT_TRY(derive_options(options, &opt));
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
    PT_TRY(prepare_views(cameras, base_seeds, n_views, options, &tiles, &views));
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
    if(f->holding() && f->target_reached) {
        report_tiles();
        uint64_t left = 0, held = 0;
        for(const auto &r : f->reps) {
            left += r->n_todo;
            held += r->n_held;
        }
        return fail(PT_ERR_CANCELLED, noise_reached_message(held, left));
    }
    RenderStop stop(ctl, start);
    // progress over the whole frame, serialised over the replicas (as pt_render_tiles_multi)
    SharedProgress shared(progress, progress_user, static_cast<int>(f->tiles_done), static_cast<int>(f->tiles.size()));
    // A plain frame makes one launch per replica that has work.  A progressive frame makes one per pass: every replica runs the pass over its
    // own tiles up to the frame's target, and the next pass starts when all of them have ended theirs.
    FrameRound round;
    int passes_this_call = 0;
    bool pass_limit = false;
    uint64_t noise_held = 0, noise_left = 0;
    for(;;) {
        int32_t yield_at = 0;
        if(f->quantum > 0) {
            yield_at = f->pass_in_progress ? f->target : (f->target > INT32_MAX - f->quantum ? INT32_MAX : f->target + f->quantum);
        }
        if(f->holding()) {
            // what the target holds now, from the records: out of this pass, and a new pass does not start once enough of the frame is
            // finished or held
            uint64_t left = 0, held = 0;
            for(auto &r : f->reps) {
                const int rc = frame_resort(*f, *r, yield_at);
                if(rc != PT_OK) {
                    f->status = rc;
                    f->error = "frame failed: " + last_error();
                    return fail(f->status, f->error);
                }
                left += r->n_todo;
                held += r->n_held;
            }
            if(!f->pass_in_progress && static_cast<double>(f->streams_total - left + held) >= static_cast<double>(f->noise_fraction) * static_cast<double>(f->streams_total)) {
                f->target_reached = true;
                noise_held = held;
                noise_left = left;
                break;
            }
        }
        else {
            for(auto &r : f->reps) {
                r->n_held = 0;
            }
        }
        if(f->quantum > 0) {
            f->target = yield_at;
            f->pass_in_progress = true;
        }
        PT_TRY(frame_round(f, out_image, stats, &shared, &stop, ctl, yield_at, &round));
        if(yield_at == 0) {
            break;
        }
        // the pass has ended when every stream that is left has its samples or is held (a stop that came too late to drop anything ends it too)
        const bool pass_done = round.at_target + round.held == round.left;
        if(pass_done) {
            f->pass_in_progress = false;
            f->passes_completed++;
            passes_this_call++;
        }
        if(round.left == 0 || !pass_done) {
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
    if(f->target_reached) {
        return fail(PT_ERR_CANCELLED, noise_reached_message(noise_held, noise_left));
    }
    if(round.left != 0) {
        const std::string why = pass_limit ? "pass limit reached" : (__atomic_load_n(&stop.ctl->cancel, __ATOMIC_ACQUIRE) != 0 ? "cancelled" : "budget spent");
        return fail(PT_ERR_CANCELLED, "frame stopped (" + why + "): " + std::to_string(round.parked) + " streams parked, " + std::to_string(round.left) + " streams left");
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
    f->target_reached = false;
    if(quantum == 0) {
        f->pass_in_progress = false; // (what an interrupted pass left is a plain frame's work now)
    }
    return PT_OK;
}

int pt_frame_set_feature_params(pt_frame *f, const pt_feature_params *params) {
    if(f == nullptr) {
        return fail(PT_ERR_INVALID, "null frame");
    }
    pt_feature_params follow{};
    if(params != nullptr) {
        PT_TRY(feature_params_resolve(params, &f->options, &follow)); // (the options of a frame never change)
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    if(f->status != PT_OK) {
        return fail(f->status, f->error);
    }
    f->follow_features = params != nullptr;
    f->feature_params = follow;
    for(auto &r : f->reps) {
        r->pv_features_ready = false; // the next denoised preview computes its features again
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

// pt_frame_preview, step 1: every replica gathers its work list on its own device; the other replicas' entries come to the host
static int preview_gather(pt_frame *f, std::vector<std::vector<F4>> &far_rgba, std::vector<std::vector<int2>> &far_at) {
    const int32_t width = f->options.image_width;
    for(size_t i = 0; i < f->reps.size(); i++) {
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
        if(pt_launch_frame_gather(s->stream, r.d_todo[r.cur].ptr, r.n_todo, r.n_parked, r.d_park[r.pcur].ptr, r.d_tiles.ptr, r.d_offset.ptr,
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
    return PT_OK;
}

// pt_frame_preview, step 2, on replica 0's device (its render_mutex held): the caller's image, the holes no tile covers, every replica's
// entries over them -- the view of n pixels in r0.pv_view, its sample counts in r0.pv_samples
static int preview_compose(pt_frame *f, const float *image, size_t n, const std::vector<std::vector<F4>> &far_rgba, const std::vector<std::vector<int2>> &far_at) {
    pt_frame::Replica &r0 = *f->reps[0];
    hipStream_t st = r0.s->stream;
    const int32_t width = f->options.image_width;
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
    for(size_t i = 0; i < f->reps.size(); i++) {
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
    return PT_OK;
}

static int variance_gather(pt_frame *f, const PtDevOptions &opt, std::vector<std::vector<F4>> &far_var, std::vector<std::vector<int32_t>> &far_at);
static int variance_compose(pt_frame *f, size_t n, const std::vector<std::vector<F4>> &far_var, const std::vector<std::vector<int32_t>> &far_at);

// pt_frame_preview (sigma_measured == nullptr) and pt_frame_preview_measured: `dp` is the filter's parameters when `denoise`
static int frame_preview(pt_frame *f, const float *image, bool denoise, const PtDenoiseParams &dp, const float *sigma_measured, float *out_rgba,
                         int32_t *out_samples) {
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
    std::vector<std::vector<F4>> far_rgba(f->reps.size());
    std::vector<std::vector<int2>> far_at(f->reps.size());
    PT_TRY(preview_gather(f, far_rgba, far_at));
    std::vector<std::vector<F4>> far_var(f->reps.size());
    std::vector<std::vector<int32_t>> far_var_at(f->reps.size());
    if(sigma_measured != nullptr) {
        PtDevOptions opt;
        PT_TRY(derive_options(&f->options, &opt));
        PT_TRY(variance_gather(f, opt, far_var, far_var_at));
    }
    pt_frame::Replica &r0 = *f->reps[0];
    pt_scene *s0 = r0.s;
    std::lock_guard<std::mutex> lock(s0->render_mutex);
    PT_HIP(hipSetDevice(s0->device));
    hipStream_t st = s0->stream;
    PT_TRY(preview_compose(f, image, n, far_rgba, far_at));
    float4 *view = reinterpret_cast<float4 *>(r0.pv_view.ptr);
    // 3. the filter, and the view back to the caller
    std::unique_lock<std::mutex> ws_lock;
    Event begin, end;
    if(denoise) {
        if(!r0.pv_features_ready) {
            PT_HIP(r0.pv_features.ensure(3 * n));
            PT_TRY(features_views_launch(s0, f->n_views > 1 ? f->cameras.data() : &f->camera, f->n_views, &f->options, reinterpret_cast<float4 *>(r0.pv_features.ptr),
                                         f->follow_features ? &f->feature_params : nullptr));
            r0.pv_features_ready = true;
        }
        DenoiseWorkspace &ws = denoise_workspace(s0->device);
        ws_lock = std::unique_lock<std::mutex>(ws.mutex); // (held until the stream has been synchronised below)
        PT_TRY(denoise_ensure(ws, n, false));
        // (one view: pt_denoise_masked_run itself; more: its view form, a hole filled from its own view only)
        if(sigma_measured != nullptr) {
            PT_TRY(variance_compose(f, n, far_var, far_var_at));
        }
        PT_HIP(begin.create());
        PT_HIP(end.create());
        PT_HIP(hipEventRecord(begin.e, st));
        if(sigma_measured != nullptr) {
            PT_HIP(pt_denoise_measured_run(st, view, reinterpret_cast<const float4 *>(r0.pv_features.ptr), reinterpret_cast<const float4 *>(r0.vr_map.ptr),
                                           r0.pv_samples.ptr, width, height, dp, *sigma_measured, ws.scratch, view));
        }
        else {
            PT_HIP(pt_denoise_views_run(st, view, reinterpret_cast<const float4 *>(r0.pv_features.ptr), r0.pv_samples.ptr, width, height, f->n_views, dp, ws.scratch, view));
        }
        PT_HIP(hipEventRecord(end.e, st));
    }
    PT_HIP(hipMemcpyAsync(out_rgba, view, n * sizeof(F4), hipMemcpyDeviceToHost, st));
    if(out_samples != nullptr) {
        PT_HIP(hipMemcpyAsync(out_samples, r0.pv_samples.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    PT_HIP(hipStreamSynchronize(st));
    if(denoise) {
        float ms = 0.0f;
        PT_HIP(hipEventElapsedTime(&ms, begin.e, end.e));
        f->preview_filter_ms = ms;
    }
    return PT_OK;
}

extern "C" int pt_frame_preview(pt_frame *f, const float *image, const pt_denoise_params *denoise, float *out_rgba, int32_t *out_samples) {
    if(f == nullptr || image == nullptr || out_rgba == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    PtDenoiseParams dp{};
    if(denoise != nullptr) {
        PT_TRY(denoise_params_resolve(denoise, &dp));
    }
    return frame_preview(f, image, denoise != nullptr, dp, nullptr, out_rgba, out_samples);
}

// ---- the noise of a frame (pt_frame_get_noise, pt_frame_set_noise_target; include/pt_frame_noise.h) -------------------------------------

extern "C" int pt_frame_set_noise_target(pt_frame *f, float target_error, float floor, float fraction) {
    if(f == nullptr) {
        return fail(PT_ERR_INVALID, "null frame");
    }
    if(!std::isfinite(target_error) || target_error < 0.0f) {
        return fail(PT_ERR_INVALID, "the target error must be finite and not negative");
    }
    if(!std::isfinite(floor) || floor < 0.0f) {
        return fail(PT_ERR_INVALID, "the floor must be finite and not negative");
    }
    if(!(fraction > 0.0f && fraction <= 1.0f)) {
        return fail(PT_ERR_INVALID, "the fraction must be in (0, 1]");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    if(f->status != PT_OK) {
        return fail(f->status, f->error);
    }
    f->noise_target = target_error;
    f->noise_floor = floor;
    f->noise_fraction = fraction;
    f->target_reached = false;
    return PT_OK;
}

// pt_frame_get_noise, step 1: every replica that has rendered rates its work list on its own device; the summaries, and the other
// replicas' entries when a map is wanted, come to the host
static int noise_rate(pt_frame *f, const PtNoiseRule &rule, bool want_map, std::vector<std::vector<uint32_t>> &summary, std::vector<std::vector<uint2>> &far) {
    f->noise_rate_ms = 0.0;
    for(size_t i = 0; i < f->reps.size(); i++) {
        pt_frame::Replica &r = *f->reps[i];
        if(!r.ready || r.n_todo == 0) {
            continue;
        }
        pt_scene *s = r.s;
        std::lock_guard<std::mutex> lock(s->render_mutex);
        PT_HIP(hipSetDevice(s->device));
        PT_HIP(r.nz_rated.ensure(r.n_todo));
        PT_HIP(r.nz_summary.ensure(PT_NOISE_SUMMARY_WORDS));
        Event begin, end;
        PT_HIP(begin.create());
        PT_HIP(end.create());
        PT_HIP(hipEventRecord(begin.e, s->stream));
        if(pt_launch_frame_rate(s->stream, r.d_todo[r.cur].ptr, r.n_todo, r.d_park[r.pcur].ptr, r.d_tiles.ptr, r.d_offset.ptr, static_cast<uint32_t>(r.tiles.size()),
                                f->options.image_width, rule, r.nz_rated.ptr, r.nz_summary.ptr) != 0) {
            PT_HIP(hipGetLastError());
            return fail(PT_ERR_HIP, "noise: rating kernel failed to launch");
        }
        PT_HIP(hipEventRecord(end.e, s->stream));
        summary[i].resize(PT_NOISE_SUMMARY_WORDS);
        PT_HIP(hipMemcpyAsync(summary[i].data(), r.nz_summary.ptr, PT_NOISE_SUMMARY_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        if(want_map && i != 0) {
            far[i].resize(r.n_todo);
            PT_HIP(hipMemcpyAsync(far[i].data(), r.nz_rated.ptr, r.n_todo * sizeof(uint2), hipMemcpyDeviceToHost, s->stream));
        }
        PT_HIP(hipStreamSynchronize(s->stream));
        float ms = 0.0f;
        PT_HIP(hipEventElapsedTime(&ms, begin.e, end.e));
        f->noise_rate_ms += ms;
    }
    return PT_OK;
}

// pt_frame_get_noise, step 2, on replica 0's device (its render_mutex held), as preview_compose: finished (-1) where a tile of a replica
// that has rendered covers the pixel, +inf elsewhere, every replica's entries over them -- the map of n pixels in r0.nz_map
static int noise_compose(pt_frame *f, size_t n, const std::vector<std::vector<uint2>> &far) {
    pt_frame::Replica &r0 = *f->reps[0];
    hipStream_t st = r0.s->stream;
    const int32_t width = f->options.image_width;
    r0.previewed = true; // (replica 0's device holds buffers of the frame now, whether or not the replica has rendered)
    PT_HIP(r0.nz_map.ensure(n));
    size_t ready = 0;
    for(const auto &r : f->reps) {
        ready += r->ready ? 1 : 0;
    }
    if(r0.nz_cover_ready != ready) {
        std::vector<uint8_t> cover(n, 0);
        for(const auto &r : f->reps) {
            for(const pt_tile &t : r->tiles) {
                for(int32_t y = t.y; r->ready && y < t.y + t.h; y++) {
                    std::memset(cover.data() + static_cast<size_t>(y) * width + t.x, 1, static_cast<size_t>(t.w));
                }
            }
        }
        PT_HIP(r0.nz_cover.upload(cover));
        r0.nz_cover_ready = ready;
    }
    if(pt_launch_frame_noise_base(st, r0.nz_map.ptr, r0.nz_cover.ptr, static_cast<uint32_t>(n)) != 0) {
        PT_HIP(hipGetLastError());
        return fail(PT_ERR_HIP, "noise: base kernel failed to launch");
    }
    for(size_t i = 0; i < f->reps.size(); i++) {
        const pt_frame::Replica &r = *f->reps[i];
        if(!r.ready || r.n_todo == 0) {
            continue;
        }
        const uint2 *rated = r0.nz_rated.ptr;
        if(i != 0) {
            PT_HIP(r0.nz_stage.ensure(r.n_todo));
            PT_HIP(hipMemcpyAsync(r0.nz_stage.ptr, far[i].data(), r.n_todo * sizeof(uint2), hipMemcpyHostToDevice, st));
            rated = r0.nz_stage.ptr;
        }
        if(pt_launch_frame_noise_scatter(st, rated, r.n_todo, r0.nz_map.ptr) != 0) {
            PT_HIP(hipGetLastError());
            return fail(PT_ERR_HIP, "noise: scatter kernel failed to launch");
        }
    }
    return PT_OK;
}

extern "C" int pt_frame_get_noise(pt_frame *f, pt_frame_noise *out, float *out_error) {
    if(f == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    const size_t n = static_cast<size_t>(f->options.image_width) * static_cast<size_t>(f->rows());
    if(n > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    std::lock_guard<std::mutex> frame_lock(f->mutex);
    if(f->status != PT_OK) {
        return fail(f->status, f->error);
    }
    PtDevOptions opt;
    PT_TRY(derive_options(&f->options, &opt));
    std::vector<std::vector<uint32_t>> summary(f->reps.size());
    std::vector<std::vector<uint2>> far(f->reps.size());
    PT_TRY(noise_rate(f, f->noise_rule(opt, true), out_error != nullptr, summary, far));
    std::memset(out, 0, sizeof(*out));
    out->target_error = f->noise_target;
    out->floor = f->noise_floor;
    out->fraction = f->noise_fraction;
    out->streams_total = f->streams_total;
    uint32_t max_bits = 0;
    uint64_t left = 0;
    bool any_ready = false;
    for(size_t i = 0; i < f->reps.size(); i++) {
        const pt_frame::Replica &r = *f->reps[i];
        left += r.n_todo;
        any_ready = any_ready || r.ready;
        if(summary[i].empty()) {
            out->streams_unrated += r.n_todo; // (no launch yet: its streams are untouched)
            continue;
        }
        out->streams_rated += summary[i][0];
        out->streams_unrated += summary[i][1];
        out->streams_held += summary[i][2];
        max_bits = std::max(max_bits, summary[i][3]);
        for(int b = 0; b < 64; b++) {
            out->histogram[b] += summary[i][4 + b];
        }
    }
    out->streams_finished = f->streams_total - left;
    out->max_error = from_bits(max_bits);
    out->target_reached = f->noise_target > 0.0f && static_cast<double>(out->streams_finished + out->streams_held) >=
                                                       static_cast<double>(f->noise_fraction) * static_cast<double>(f->streams_total)
                            ? 1
                            : 0;
    if(out_error == nullptr) {
        return PT_OK;
    }
    if(!any_ready) {
        std::fill(out_error, out_error + n, std::numeric_limits<float>::infinity()); // (before the first pt_frame_render every pixel is untouched)
        return PT_OK;
    }
    pt_scene *s0 = f->reps[0]->s;
    std::lock_guard<std::mutex> lock(s0->render_mutex);
    PT_HIP(hipSetDevice(s0->device));
    PT_TRY(noise_compose(f, n, far));
    PT_HIP(hipMemcpyAsync(out_error, f->reps[0]->nz_map.ptr, n * sizeof(float), hipMemcpyDeviceToHost, s0->stream));
    PT_HIP(hipStreamSynchronize(s0->stream));
    return PT_OK;
}

// diagnostic (tools/noise_probe.py): the device time of the rating kernels of the frame's last pt_frame_get_noise, all replicas
extern "C" int pt_debug_frame_noise_ms(pt_frame *f, double *out_ms) {
    if(f == nullptr || out_ms == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    *out_ms = f->noise_rate_ms;
    return PT_OK;
}

// ---- the variance map of a frame (pt_frame_get_variance, pt_frame_preview_measured; include/pt_frame_variance.h) -------------------------

// step 1: every replica that has rendered gathers the measured variance of its work list on its own device; the other replicas'
// entries come to the host
static int variance_gather(pt_frame *f, const PtDevOptions &opt, std::vector<std::vector<F4>> &far_var, std::vector<std::vector<int32_t>> &far_at) {
    f->variance_gather_ms = 0.0;
    for(size_t i = 0; i < f->reps.size(); i++) {
        pt_frame::Replica &r = *f->reps[i];
        if(!r.ready || r.n_todo == 0) {
            continue;
        }
        pt_scene *s = r.s;
        std::lock_guard<std::mutex> lock(s->render_mutex);
        PT_HIP(hipSetDevice(s->device));
        r.previewed = true;
        PT_HIP(r.vr_var.ensure(r.n_todo));
        PT_HIP(r.vr_at.ensure(r.n_todo));
        Event begin, end;
        PT_HIP(begin.create());
        PT_HIP(end.create());
        PT_HIP(hipEventRecord(begin.e, s->stream));
        if(pt_launch_frame_variance(s->stream, r.d_todo[r.cur].ptr, r.n_todo, r.d_park[r.pcur].ptr, r.d_tiles.ptr, r.d_offset.ptr, static_cast<uint32_t>(r.tiles.size()),
                                    f->options.image_width, opt, reinterpret_cast<float4 *>(r.vr_var.ptr), r.vr_at.ptr) != 0) {
            PT_HIP(hipGetLastError());
            return fail(PT_ERR_HIP, "variance: gather kernel failed to launch");
        }
        PT_HIP(hipEventRecord(end.e, s->stream));
        if(i != 0) {
            far_var[i].resize(r.n_todo);
            far_at[i].resize(r.n_todo);
            PT_HIP(hipMemcpyAsync(far_var[i].data(), r.vr_var.ptr, r.n_todo * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
            PT_HIP(hipMemcpyAsync(far_at[i].data(), r.vr_at.ptr, r.n_todo * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        }
        PT_HIP(hipStreamSynchronize(s->stream));
        float ms = 0.0f;
        PT_HIP(hipEventElapsedTime(&ms, begin.e, end.e));
        f->variance_gather_ms += ms;
    }
    return PT_OK;
}

// step 2, on replica 0's device (its render_mutex held), as preview_compose: zeros, every replica's entries over them -- the map of n
// pixels in r0.vr_map
static int variance_compose(pt_frame *f, size_t n, const std::vector<std::vector<F4>> &far_var, const std::vector<std::vector<int32_t>> &far_at) {
    pt_frame::Replica &r0 = *f->reps[0];
    hipStream_t st = r0.s->stream;
    r0.previewed = true;
    PT_HIP(r0.vr_map.ensure(n));
    PT_HIP(hipMemsetAsync(r0.vr_map.ptr, 0, n * sizeof(F4), st)); // (the base: finished, untouched and uncovered pixels are (0, 0, 0, 0))
    for(size_t i = 0; i < f->reps.size(); i++) {
        const pt_frame::Replica &r = *f->reps[i];
        if(!r.ready || r.n_todo == 0) {
            continue;
        }
        const float4 *var = reinterpret_cast<const float4 *>(r0.vr_var.ptr);
        const int32_t *at = r0.vr_at.ptr;
        if(i != 0) {
            PT_HIP(r0.vr_stage_var.ensure(r.n_todo));
            PT_HIP(r0.vr_stage_at.ensure(r.n_todo));
            PT_HIP(hipMemcpyAsync(r0.vr_stage_var.ptr, far_var[i].data(), r.n_todo * sizeof(F4), hipMemcpyHostToDevice, st));
            PT_HIP(hipMemcpyAsync(r0.vr_stage_at.ptr, far_at[i].data(), r.n_todo * sizeof(int32_t), hipMemcpyHostToDevice, st));
            var = reinterpret_cast<const float4 *>(r0.vr_stage_var.ptr);
            at = r0.vr_stage_at.ptr;
        }
        if(pt_launch_frame_variance_scatter(st, var, at, r.n_todo, reinterpret_cast<float4 *>(r0.vr_map.ptr)) != 0) {
            PT_HIP(hipGetLastError());
            return fail(PT_ERR_HIP, "variance: scatter kernel failed to launch");
        }
    }
    return PT_OK;
}

extern "C" int pt_frame_get_variance(pt_frame *f, float *out_var) {
    if(f == nullptr || out_var == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    const size_t n = static_cast<size_t>(f->options.image_width) * static_cast<size_t>(f->rows());
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
        std::memset(out_var, 0, n * sizeof(F4)); // (before the first pt_frame_render every pixel is untouched)
        return PT_OK;
    }
    PtDevOptions opt;
    PT_TRY(derive_options(&f->options, &opt));
    std::vector<std::vector<F4>> far_var(f->reps.size());
    std::vector<std::vector<int32_t>> far_at(f->reps.size());
    PT_TRY(variance_gather(f, opt, far_var, far_at));
    pt_scene *s0 = f->reps[0]->s;
    std::lock_guard<std::mutex> lock(s0->render_mutex);
    PT_HIP(hipSetDevice(s0->device));
    PT_TRY(variance_compose(f, n, far_var, far_at));
    PT_HIP(hipMemcpyAsync(out_var, f->reps[0]->vr_map.ptr, n * sizeof(F4), hipMemcpyDeviceToHost, s0->stream));
    PT_HIP(hipStreamSynchronize(s0->stream));
    return PT_OK;
}

extern "C" int pt_frame_preview_measured(pt_frame *f, const float *image, const pt_denoise_measured_params *params, float *out_rgba, int32_t *out_samples) {
    if(f == nullptr || image == nullptr || out_rgba == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    PtDenoiseParams dp{};
    float sigma_measured = 0.0f;
    PT_TRY(denoise_measured_params_resolve(params, &dp, &sigma_measured));
    if(f->n_views > 1) {
        return fail(PT_ERR_UNSUPPORTED, "a view frame has no measured preview");
    }
    return frame_preview(f, image, true, dp, &sigma_measured, out_rgba, out_samples);
}

// diagnostic (tools/measured_probe.py): the device time of the gather kernels of the frame's last variance map, all replicas, and of the
// filter of its last denoised preview (either may be NULL)
extern "C" int pt_debug_frame_measured_ms(pt_frame *f, double *out_gather_ms, double *out_filter_ms) {
    if(f == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    if(out_gather_ms != nullptr) {
        *out_gather_ms = f->variance_gather_ms;
    }
    if(out_filter_ms != nullptr) {
        *out_filter_ms = f->preview_filter_ms;
    }
    return PT_OK;
}
