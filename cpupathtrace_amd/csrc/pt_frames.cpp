// pt_frames.cpp -- resumable frames of the C ABI (include/pt_hip.h): pt_frame_create*, pt_frame_render and its progressive passes, the
// frame's settings and queries.  The maps of an unfinished frame (preview, noise, variance) are pt_frame_maps.cpp.
#include "pt_frames.h"

using namespace pth;

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
    PT_HIP(r.d_result.ensure(PT_COMPACT_WORDS));
    r.ready = true;
    return PT_OK;
}

// The replica's next work list (its render_mutex held), on the host when this returns: the compaction's result words and, with `left`,
// the tiles' counts of unfinished pixels.  resort: nothing was launched, the list as it stands is split again and its records stay;
// otherwise from what the launch left, its records in d_park[pcur ^ 1], `cap` of them at most.
int frame_compact(const pt_frame &f, pt_frame::Replica &r, const PtDevOptions &opt, int32_t target, bool resort, uint32_t cap, unsigned long long *res,
                  std::vector<uint32_t> *left) {
    hipStream_t st = r.s->stream;
    const PtParkRecord *park_in = r.d_park[r.pcur].ptr;
    PtParkRecord *park_out = resort ? nullptr : r.d_park[r.pcur ^ 1].ptr;
    PT_LAUNCH(pt_launch_frame_compact(st, r.d_todo[r.cur].ptr, r.n_todo, r.d_status.ptr, resort ? park_in : park_out, r.d_todo[r.cur ^ 1].ptr, r.d_blocks.ptr, r.d_result.ptr,
                                      target, park_in, park_out, resort ? nullptr : r.d_park_count.ptr, cap, f.noise_rule(opt, resort || f.holding()), resort ? 1 : 0),
              "frame: work list kernel failed to launch");
    PT_HIP(hipMemcpyAsync(res, r.d_result.ptr, PT_COMPACT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if(left != nullptr) {
        left->resize(r.tiles.size());
        PT_HIP(hipMemcpyAsync(left->data(), r.d_left.ptr, left->size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    PT_HIP(hipStreamSynchronize(st));
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
    unsigned long long res[PT_COMPACT_WORDS];
    std::vector<uint32_t> left;
    PT_TRY(frame_compact(f, r, opt, progressive ? yield_at : 0, false, cap, res, &left));
    // every stream of the work list is finished, parked or still to do, and the stop dropped no more than the parked and returned ones
    // (a progressive pass drops no record: no sample found no room)
    const StreamTally &t = out->tally;
    const unsigned long long first = res[PT_COMPACT_FIRST], second = res[PT_COMPACT_SECOND], held = res[PT_COMPACT_HELD], written = res[PT_COMPACT_WRITTEN];
    if(t.finished + first + second + held != r.n_todo || written > t.abandoned || res[PT_COMPACT_WITH_RECORD] > cap || (!progressive && written != first) ||
       res[PT_COMPACT_NO_ROOM] != 0) {
        return fail(PT_ERR_HIP, "frame: " + std::to_string(t.finished) + " finished, " + std::to_string(first) + " parked and " + std::to_string(second) +
                                    " left of " + std::to_string(r.n_todo) + " streams (" + std::to_string(t.abandoned) + " dropped, " + std::to_string(held) + " held)");
    }
    r.n_todo = static_cast<uint32_t>(first + second + held);
    r.n_parked = static_cast<uint32_t>(res[PT_COMPACT_WITH_RECORD]);
    r.n_held = static_cast<uint32_t>(held);
    r.in_order = r.n_todo == r.n_streams && (r.n_parked == 0 || r.n_parked == r.n_todo) && (!progressive || std::max({first, second, held}) == r.n_todo); // (each part in order)
    r.samples_carried = res[PT_COMPACT_CARRIED];
    r.with_candidates = res[PT_COMPACT_WITH_CANDIDATES];
    r.n_at_target = progressive ? static_cast<uint32_t>(second) : 0;
    r.min_samples = r.n_todo != 0 ? static_cast<int32_t>(0xffffffffULL - res[PT_COMPACT_MIN_INVERTED]) : 0;
    r.max_samples = static_cast<int32_t>(res[PT_COMPACT_MAX]);
    r.cur = next;
    r.pcur = pnext;
    out->parked = written;
    for(size_t k = 0; k < left.size(); k++) {
        f.tile_done[r.index[k]] = left[k] == 0 ? 1 : 0;
    }
    return PT_OK;
}

} // namespace

// A progressive frame with a noise target, before a pass to `yield_at` samples: the replica's list split again by that sample count and
// the target as they are now -- streams below the count, streams at it, held streams -- with nothing launched and no record moved.
// (declared in pt_frames.h: a loaded checkpoint splits the list it rebuilt with it, pt_checkpoint.cpp)
int pth::frame_resort(pt_frame &f, pt_frame::Replica &r, int32_t yield_at) {
    if(!r.ready || r.n_todo == 0) {
        r.n_held = 0; // (no records yet: nothing is rated)
        return PT_OK;
    }
    pt_scene *s = r.s;
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtDevOptions opt;
    PT_TRY(derive_options(&f.options, &opt));
    unsigned long long res[PT_COMPACT_WORDS];
    PT_TRY(frame_compact(f, r, opt, yield_at, true, 0, res, nullptr));
    const unsigned long long first = res[PT_COMPACT_FIRST], second = res[PT_COMPACT_SECOND], held = res[PT_COMPACT_HELD];
    if(first + second + held != r.n_todo) {
        return fail(PT_ERR_HIP, "frame: " + std::to_string(first + second) + " streams to do and " + std::to_string(held) + " held of " + std::to_string(r.n_todo));
    }
    r.in_order = r.in_order && std::max({first, second, held}) == r.n_todo;
    r.n_at_target = static_cast<uint32_t>(second);
    r.n_held = static_cast<uint32_t>(held);
    r.cur ^= 1;
    return PT_OK;
}

namespace {

// A failure of a launch or of a work list fails the frame for good: every later call returns this
int frame_fail(pt_frame *f, int rc) {
    f->status = rc;
    f->error = "frame failed: " + last_error();
    return fail(f->status, f->error);
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
        return frame_fail(f, rc);
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
        r->s->live_frames.fetch_add(1); // (pt_scene_pose refuses a scene that has a frame; pt_frame_destroy counts down)
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
    PT_TRY(f->check());
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
                    return frame_fail(f, rc);
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
    PT_TRY(f->check());
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
    PT_TRY(f->check());
    f->follow_features = params != nullptr;
    f->feature_params = follow;
    for(auto &r : f->reps) {
        r->pv_features_ready = false; // the next denoised preview computes its features again
    }
    return PT_OK;
}

// (include/pt_frame_noise.h)
int pt_frame_set_noise_target(pt_frame *f, float target_error, float floor, float fraction) {
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
    PT_TRY(f->check());
    f->noise_target = target_error;
    f->noise_floor = floor;
    f->noise_fraction = fraction;
    f->target_reached = false;
    return PT_OK;
}

int pt_frame_get_progress(const pt_frame *f, pt_frame_progress *out) {
    if(f == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    PT_TRY(f->check());
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
            r->s->live_frames.fetch_sub(1);
            r.reset();
        }
    }
    delete f;
    return PT_OK;
}

} // extern "C"
