// pt_render.cpp -- the render calls of the C ABI (include/pt_hip.h): the workspace and the launch of the persistent path kernel
// (pt_path.hip: one launch per call and scene), the stream, item, tile and view entry points with their multi-device, controlled and
// device-memory forms, and the pt_debug_* diagnostics.
#include "pt_host.h"

namespace pth {

int setup_path(pt_scene *s) {
    PtPathConfig &cfg = s->path_cfg;
    if(cfg.rows != 0) {
        return PT_OK;
    }
    cfg.in_lds = (s->dev.n_lds_pairs == s->dev.n_pairs && s->dev.n_lds_tris == s->dev.n_tris && s->dev.n_lds_pairs + s->dev.n_lds_tris > 0) ? 1 : 0;
    // 8 stack entries per lane in LDS (16 KB per workgroup) let four workgroups share a CU; deeper walks use the HBM spill area.  A scene
    // staged in LDS that leaves no room for four workgroups that way gets a window of 4 entries (pt_trace.h, PT_PATH_STACK_LDS_SMALL)
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

namespace {

// the buffers of a grid of `waves` wavefronts with `total` slots and rings of `cap` rays; their addresses go into *cfg
int ensure_path_buffers(pt_scene *s, PtPathConfig &cfg, uint32_t waves, uint32_t total, uint32_t cap, uint32_t rays_per_slot, int ring_log) {
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
    return PT_OK;
}

} // namespace

// Grid and slot rows for n streams, and the buffers they need.
int ensure_path_workspace(pt_scene *s, uint32_t n, PtPathConfig *out_cfg, const PathPlan *plan) {
    PT_TRY(setup_path(s));
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
    // Swept again with the rare step as straight-line code, a third cheaper (profiles/slow_step_leaf_min_sweep.txt; 2 / 4 / 6 / 8 / 12 / 16): benchmark frame
    // 445 / 475 / 489 / 490 / 492 / 480, Box 1403 / 1413 / 1428 / 1444 / 1458 / 1473, Cornell 772 / 795 / 813 / 827 / 851 / 865 Msamples/s.  The optimum did
    // not move: 8 against 12 on the benchmark frame is less than one run differs from the next (spreads of 1.5 - 3.9), the scenes in LDS still want 16.
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
    PT_TRY(ensure_path_buffers(s, cfg, waves, total, cap, rays_per_slot, ring_log));
    s->path_slots = total;
    s->path_waves = waves;
    s->path_cap = cap;
    s->path_cfg.burst_steps = cfg.burst_steps; // (the diagnostics that follow a render -- pt_debug_replay_rays -- run with its settings)
    s->path_cfg.leaf_min = cfg.leaf_min;
    *out_cfg = cfg;
    return PT_OK;
}

RenderStop::RenderStop(pt_render_control *ctl_, Clock::time_point start) : ctl(ctl_ != nullptr ? ctl_ : &none) {
    if(ctl->budget_ms > 0.0) {
        has_deadline = true;
        deadline = start + std::chrono::duration_cast<Clock::duration>(std::chrono::duration<double, std::milli>(ctl->budget_ms));
    }
    poll();
}

void RenderStop::enlist(uint32_t *word) {
    std::lock_guard<std::mutex> lock(mutex);
    __atomic_store_n(word, requested.load() ? 1U : 0U, __ATOMIC_SEQ_CST);
    words.push_back(word);
}

void RenderStop::retire(uint32_t *word, Clock::time_point end) {
    std::lock_guard<std::mutex> lock(mutex);
    words.erase(std::remove(words.begin(), words.end(), word), words.end());
    if(requested.load()) {
        drain_ms = std::max(drain_ms, std::chrono::duration<double, std::milli>(end - requested_at).count());
    }
}

void RenderStop::poll() {
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

namespace {

// Streams of a launch that no wavefront took: the first round (streams 0 .. first_total-1) is always dealt out, beyond it the final value
// of the pull counter says how many were handed out (it may overshoot the job: a wavefront's last pull asks for a whole row)
uint64_t unclaimed_streams(uint64_t n, uint64_t first_total, uint64_t pulled) {
    const uint64_t first = std::min(n, first_total);
    return n - first - std::min(pulled, n - first);
}

// Every stream of a launch of n is finished or, in a controlled launch, abandoned or never taken
int check_tally(bool controlled, const StreamTally &t, uint64_t n) {
    if(controlled && t.finished + t.abandoned + t.unclaimed != n) {
        return fail(PT_ERR_HIP, "path kernel ended with " + std::to_string(t.finished) + " finished, " + std::to_string(t.abandoned) + " abandoned and " +
                                    std::to_string(t.unclaimed) + " unclaimed of " + std::to_string(n) + " streams");
    }
    if(!controlled && t.finished != n) {
        return fail(PT_ERR_HIP, "path kernel ended with " + std::to_string(t.finished) + " of " + std::to_string(n) + " streams finished");
    }
    return PT_OK;
}

} // namespace

int finish_path(pt_scene *s, StreamTally *tally) {
    PT_HIP(hipStreamSynchronize(s->stream));
    if(s->host_streams_done == nullptr || s->streams_expected == 0) {
        return PT_OK;
    }
    const volatile unsigned long long *h = static_cast<volatile unsigned long long *>(s->host_streams_done);
    const uint64_t expected = s->streams_expected;
    const bool controlled = s->streams_controlled;
    s->streams_expected = 0;
    s->streams_controlled = false;
    StreamTally t;
    t.finished = h[0];
    if(controlled) {
        t.abandoned = h[1];
        t.unclaimed = unclaimed_streams(expected, s->streams_first_total, static_cast<uint32_t>(h[2]));
    }
    const int rc = check_tally(controlled, t, expected);
    if(rc == PT_OK && controlled && tally != nullptr) {
        *tally = t;
    }
    return rc;
}

// ---- run_path: placement, arguments, launch, host loop, statistics ------------------------------------------------------------------

namespace {

// pt_debug_set_place: the scene's table is the first round of this launch only (plan->d_place stays null without one)
int path_placement(pt_scene *s, PathPlan *plan) {
    if(s->debug_place.empty()) {
        return PT_OK;
    }
    PT_HIP(s->place.ensure(s->debug_place.size()));
    PT_HIP(hipMemcpyAsync(s->place.ptr, s->debug_place.data(), s->debug_place.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    plan->waves = s->debug_place_waves;
    plan->slots_per_wave = s->debug_place_slots;
    plan->d_place = s->place.ptr;
    s->debug_place.clear();
    return PT_OK;
}

// What the launch is told about its streams beyond the caller's T: the first round over the workspace's grid, the cost table of
// pt_debug_collect_costs and, with a host loop (`watched`: a progress function or a stop), where the kernel counts finished tiles.
int path_arguments(pt_scene *s, const PtPathConfig &cfg, const PathPlan *plan, bool watched, PtStreams *streams) {
    PtStreams &T = *streams;
    T.place = plan != nullptr ? plan->d_place : nullptr;
    T.cost = nullptr;
    if(s->debug_collect_costs) {
        PT_HIP(s->stream_cost.ensure(std::max<uint32_t>(T.n, 1U)));
        T.cost = s->stream_cost.ptr;
    }
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
    if(watched && T.rect == nullptr && T.n_tiles > 0) {
        if(s->host_tiles_done == nullptr) {
            PT_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->host_tiles_done), 64, hipHostMallocDefault));
        }
        *s->host_tiles_done = 0;
        T.tiles_done = s->host_tiles_done;
        T.tile_left = own_left != nullptr ? own_left : s->tile_left.ptr; // filled by the caller (pixels per tile)
    }
    return PT_OK;
}

// From here until the host loop has seen the launch end (or run_path returns), a stop request reaches this launch
struct Enlisted {
    RenderStop *stop = nullptr;
    uint32_t *word = nullptr;
    ~Enlisted() {
        if(stop != nullptr) {
            stop->retire(word, RenderStop::Clock::now());
        }
    }
};

// The launch on the scene's stream, between its two events: cleared counters in front of it, the copies of its stream counts (finish_path)
// behind it.  A controlled launch is enlisted with its stop just before it is issued.
int path_launch(pt_scene *s, const PtDevCamera &cam, const PtDevOptions &opt, PtStreams &T, const PtPathConfig &cfg, float4 *d_image, RenderStop *stop, Event &ev_begin,
                Event &ev_end, Enlisted *enlisted) {
    hipStream_t st = s->stream;
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
    PT_HIP(hipMemsetAsync(s->counters.ptr, 0, sizeof(PtDevCounters), st));
    PT_HIP(hipMemsetAsync(s->pull_counter.ptr, 0, 64 * sizeof(uint32_t), st));
    PT_HIP(hipMemsetAsync(s->path_wave_counters.ptr, 0, static_cast<size_t>(s->path_waves) * 8U * sizeof(unsigned long long), st));
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
        enlisted->stop = stop;
        enlisted->word = s->host_cancel;
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
    return PT_OK;
}

// The host loop of a watched launch: reports every finished tile from the calling thread and forwards a stop request, until the launch ends
int path_host_loop(pt_scene *s, const PtStreams &T, Event &ev_end, pt_progress_fn progress, void *progress_user, RenderStop *stop, Enlisted *enlisted) {
    const int total = static_cast<int>(T.n_tiles);
    int reported = 0;
    for(;;) {
        // (the count is read after the query: what a finished launch counted is all there, and the last turn reports the rest)
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
        enlisted->stop = nullptr;
    }
    return PT_OK;
}

// PT_DEBUG: how the launch's steps spread over its wavefronts (a wavefront's busy time follows its steps; the launch lasts as long as the busiest one)
void print_path_stats(const pt_scene *s, const PtPathConfig &cfg, float ms, const unsigned long long *sum, const std::vector<unsigned long long> &slots) {
    std::fprintf(stderr, "[pt] path kernel: %.2f ms, grid %d x 256, %d rows; wave steps %llu (%.1f lanes of 64 busy per step), shading passes %llu, rays %llu\n", ms, cfg.grid,
                 cfg.rows, sum[4], sum[4] ? static_cast<double>(sum[0] + sum[1]) / static_cast<double>(sum[4]) : 0.0, sum[5], sum[2]);
    std::vector<unsigned long long> steps(s->path_waves);
    for(size_t w = 0; w < steps.size(); w++) {
        steps[w] = slots[8 * w + 4] & 0xffffffffULL;
    }
    std::sort(steps.begin(), steps.end());
    const double mean = static_cast<double>(sum[4]) / static_cast<double>(steps.size());
    std::fprintf(stderr, "[pt] wave steps per wavefront: mean %.0f, min %llu, median %llu, 90 %% %llu, 99 %% %llu, max %llu (max / mean %.3f)\n", mean, steps.front(),
                 steps[steps.size() / 2], steps[steps.size() * 9 / 10], steps[steps.size() * 99 / 100], steps.back(), static_cast<double>(steps.back()) / mean);
}

// Waits for the launch and reads what it counted: the wavefronts' counters summed into *stats, after the check that every stream is accounted for
int path_stats(pt_scene *s, const PtStreams &T, const PtPathConfig &cfg, bool controlled, Event &ev_begin, Event &ev_end, pt_stats *stats) {
    PT_HIP(hipEventSynchronize(ev_end.e));
    float ms = 0.0F;
    PT_HIP(hipEventElapsedTime(&ms, ev_begin.e, ev_end.e));
    std::vector<unsigned long long> slots(static_cast<size_t>(s->path_waves) * 8U);
    PT_HIP(hipMemcpy(slots.data(), s->path_wave_counters.ptr, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, high[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for(size_t i = 0; i < slots.size(); i++) {
        // (a PT_PATH_TIMING build packs kilo-cycle totals and slow_step's counts into the high words; they are zero otherwise: a wavefront's counts fit 32 bits)
        const size_t k = i & 7U;
        sum[k] += slots[i] & 0xffffffffULL;
        high[k] += slots[i] >> 32;
    }
    const unsigned long long *kcycles = high + 3; // the waves' lifetimes, traversal bursts, shading passes, the inner loop
    if(kcycles[0] == 0) {
        // (not a timing build: the other four counters are whole 64-bit words)
        for(const size_t k : {size_t{0}, size_t{1}, size_t{2}, size_t{7}}) {
            sum[k] += high[k] << 32;
        }
    }
    if(kcycles[0] != 0 && env_int("PT_DEBUG", 0) != 0) {
        const double all = static_cast<double>(kcycles[0]);
        std::fprintf(stderr, "[pt] wave time: %.1f %% in shading passes, %.1f %% in traversal bursts, %.1f %% in the inner loop outside the bursts (of the waves' lifetimes; %llu kilo-cycles in all)\n",
                     100.0 * static_cast<double>(kcycles[2]) / all, 100.0 * static_cast<double>(kcycles[1]) / all,
                     100.0 * (static_cast<double>(kcycles[3]) - static_cast<double>(kcycles[1])) / all, kcycles[0]);
        // the rare step's part of the bursts: high words of slots 0, 1, 2 and 7 (kilo-cycles, invocations, lanes served, trips of the pop loop)
        const double calls = static_cast<double>(std::max<unsigned long long>(high[1], 1));
        std::fprintf(stderr, "[pt] slow_step: %.1f %% of the waves' lifetimes (%.1f %% of the bursts); %.4f invocations per wave step, %.2f lanes and %.2f pop trips per invocation (%llu invocations)\n",
                     100.0 * static_cast<double>(high[0]) / all, 100.0 * static_cast<double>(high[0]) / static_cast<double>(std::max<unsigned long long>(kcycles[1], 1)),
                     static_cast<double>(high[1]) / static_cast<double>(std::max<unsigned long long>(sum[4], 1)), static_cast<double>(high[2]) / calls,
                     static_cast<double>(high[7]) / calls, high[1]);
    }
    PtDevCounters done{};
    PT_HIP(hipMemcpy(&done, s->counters.ptr, sizeof(done), hipMemcpyDeviceToHost));
    StreamTally t;
    t.finished = done.streams_done;
    if(controlled) {
        uint32_t pulled = 0;
        PT_HIP(hipMemcpy(&pulled, s->pull_counter.ptr, sizeof(pulled), hipMemcpyDeviceToHost));
        t.abandoned = done.streams_abandoned;
        t.unclaimed = unclaimed_streams(T.n, T.first_total, pulled);
    }
    PT_TRY(check_tally(controlled, t, T.n));
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
        print_path_stats(s, cfg, ms, sum, slots);
    }
    return PT_OK;
}

} // namespace

int run_path(pt_scene *s, const PtDevCamera &cam, const PtDevOptions &opt, PtStreams T, float4 *d_image, pt_stats *stats, pt_progress_fn progress, void *progress_user,
             RenderStop *stop) {
    PathPlan placed;
    PT_TRY(path_placement(s, &placed));
    const PathPlan *plan = placed.d_place != nullptr ? &placed : nullptr;
    PtPathConfig cfg;
    PT_TRY(ensure_path_workspace(s, T.n, &cfg, plan));
    PT_TRY(path_arguments(s, cfg, plan, progress != nullptr || stop != nullptr, &T));
    Event ev_begin, ev_end;
    Enlisted enlisted;
    PT_TRY(path_launch(s, cam, opt, T, cfg, d_image, stop, ev_begin, ev_end, &enlisted));
    if(T.tiles_done != nullptr) {
        PT_TRY(path_host_loop(s, T, ev_end, progress, progress_user, stop, &enlisted));
    }
    if(stats != nullptr) {
        PT_TRY(path_stats(s, T, cfg, stop != nullptr, ev_begin, ev_end, stats));
    }
    return PT_OK;
}

} // namespace pth

using namespace pth;

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
    PT_TRY(setup_path(s));
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
    EventPair timer;
    PT_HIP(timer.begin(s->stream));
    *out_blocks = pt_launch_replay(s->stream, s->dev, Q, s->path_waves, static_cast<uint32_t>(parts), waves_per_simd, cfg, s->path_spill.ptr, s->path_wave_counters.ptr);
    PT_HIP(hipGetLastError());
    PT_HIP(timer.end(s->stream));
    PT_HIP(hipMemcpyAsync(out, s->path_wave_counters.ptr, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    PT_HIP(timer.ms(out_ms));
    return PT_OK;
}

extern "C" {

int pt_render_streams(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_stream *streams, size_t n, float *out_image,
                      uint64_t *out_states, pt_stats *stats) {
    PT_TRY(check_render_args(s, camera, options));
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
    PT_TRY(derive_options(options, &opt));
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
        const int rc = run_path(s, cam, opt, T, reinterpret_cast<float4 *>(s->image.ptr), stats, nullptr, nullptr);
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

} // extern "C"

namespace pth {

void tile_grid(const pt_tile *tiles, size_t n_tiles, uint32_t *tiles_per_row, uint32_t *chunks_per_tile) {
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

int check_tiles(const pt_tile *tiles, size_t n_tiles, int32_t width, int32_t rows, uint64_t *total, const char *unit) {
    uint64_t pixels = 0;
    for(size_t k = 0; k < n_tiles; k++) {
        const pt_tile &t = tiles[k];
        if(t.w <= 0 || t.h <= 0 || t.x < 0 || t.y < 0 || t.x + t.w > width || t.y + t.h > rows) {
            return fail(PT_ERR_INVALID, "tile outside the image or empty");
        }
        pixels += static_cast<uint64_t>(t.w) * static_cast<uint64_t>(t.h);
    }
    if(total != nullptr) {
        if(pixels > 0x0fffffffULL) {
            return fail(PT_ERR_INVALID, std::string("too many pixels in one ") + unit);
        }
        *total = pixels;
    }
    return PT_OK;
}

TileTable::TileTable(const pt_tile *tiles, size_t n_tiles) : rects(n_tiles), offsets(n_tiles), left(n_tiles) {
    uint32_t at = 0;
    for(size_t k = 0; k < n_tiles; k++) {
        const pt_tile &t = tiles[k];
        rects[k] = make_int4(t.x, t.y, t.w, t.h);
        offsets[k] = at;
        left[k] = static_cast<uint32_t>(t.w) * static_cast<uint32_t>(t.h);
        at += left[k];
    }
}

void set_tile_streams(PtStreams *T, uint32_t n, const int4 *d_tiles, const uint32_t *d_offset, size_t n_tiles, uint64_t base_seed, int32_t n_views, int32_t view_height,
                      const PtViewCamera *d_view_cams, const uint64_t *d_view_seeds) {
    T->n = n;
    T->tiles = d_tiles;
    T->tile_offset = d_offset;
    T->n_tiles = static_cast<uint32_t>(n_tiles);
    T->base_seed = base_seed;
    if(n_views > 1) {
        T->n_views = static_cast<uint32_t>(n_views);
        T->view_height = static_cast<uint32_t>(view_height);
        T->views = d_view_cams;
        T->view_seed = d_view_seeds;
    }
}

} // namespace pth

// One scene's launch over a tile list (render_mutex held): the tile and view tables go to the scene's buffers, the frame is d_image
static int render_tiles_impl(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles, uint64_t base_seed,
                             float4 *d_image, pt_stats *stats, pt_progress_fn progress = nullptr, void *progress_user = nullptr, RenderStop *stop = nullptr,
                             const ViewSet *views = nullptr) {
    PtDevOptions opt;
    PT_TRY(derive_options(options, &opt));
    const PtDevCamera cam = derive_camera(camera);
    const int32_t rows = views != nullptr ? views->rows(options) : options->image_height;
    uint64_t total = 0;
    PT_TRY(check_tiles(tiles, n_tiles, options->image_width, rows, &total));
    const TileTable table(tiles, n_tiles);
    PT_HIP(s->tiles.ensure(n_tiles));
    PT_HIP(s->tile_offset.ensure(n_tiles));
    hipStream_t st = s->stream;
    PT_HIP(hipMemcpyAsync(s->tiles.ptr, table.rects.data(), n_tiles * sizeof(int4), hipMemcpyHostToDevice, st));
    PT_HIP(hipMemcpyAsync(s->tile_offset.ptr, table.offsets.data(), n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if(progress != nullptr || stop != nullptr) {
        PT_HIP(s->tile_left.ensure(n_tiles));
        PT_HIP(hipMemcpyAsync(s->tile_left.ptr, table.left.data(), n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    if(views != nullptr) {
        PT_HIP(s->view_cams.ensure(views->cams.size()));
        PT_HIP(s->view_seeds.ensure(views->seeds.size()));
        PT_HIP(hipMemcpyAsync(s->view_cams.ptr, views->cams.data(), views->cams.size() * sizeof(PtViewCamera), hipMemcpyHostToDevice, st));
        PT_HIP(hipMemcpyAsync(s->view_seeds.ptr, views->seeds.data(), views->seeds.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    PT_HIP(hipStreamSynchronize(st)); // the tables are this function's vectors
    PtStreams T{};
    set_tile_streams(&T, static_cast<uint32_t>(total), s->tiles.ptr, s->tile_offset.ptr, n_tiles, base_seed, views != nullptr ? static_cast<int32_t>(views->cams.size()) : 1,
                     options->image_height, s->view_cams.ptr, s->view_seeds.ptr);
    tile_grid(tiles, n_tiles, &T.tiles_per_row, &T.chunks_per_tile);
    return run_path(s, cam, opt, T, d_image, stats, progress, progress_user, stop);
}

extern "C" {

int pt_render_tiles(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles, uint64_t base_seed,
                    float *out_image, pt_stats *stats) {
    return pt_render_tiles_progress(s, camera, options, tiles, n_tiles, base_seed, out_image, stats, nullptr, nullptr);
}

int pt_render_tiles_progress(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles, uint64_t base_seed,
                             float *out_image, pt_stats *stats, pt_progress_fn progress, void *progress_user) {
    PT_TRY(check_render_args(s, camera, options));
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
    PT_TRY(render_tiles_impl(s, camera, options, tiles, n_tiles, base_seed, reinterpret_cast<float4 *>(s->image.ptr), stats, progress, progress_user));
    PT_HIP(hipMemcpyAsync(out_image, s->image.ptr, pixels * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
    return finish_path(s);
}

int pt_render_item(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_stream *item, float *out_tile, uint64_t *out_state,
                   pt_stats *stats) {
    PT_TRY(check_render_args(s, camera, options));
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
    PT_TRY(derive_options(options, &opt));
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
    PT_TRY(run_path(s, cam, opt, T, reinterpret_cast<float4 *>(s->image.ptr), stats, nullptr, nullptr));
    const F4 *first = s->image.ptr + static_cast<size_t>(item->y) * static_cast<size_t>(options->image_width) + static_cast<size_t>(item->x);
    PT_HIP(hipMemcpy2DAsync(out_tile, static_cast<size_t>(item->w) * sizeof(F4), first, static_cast<size_t>(options->image_width) * sizeof(F4),
                            static_cast<size_t>(item->w) * sizeof(F4), static_cast<size_t>(item->h), hipMemcpyDeviceToHost, st));
    if(out_state != nullptr) {
        PT_HIP(hipMemcpyAsync(out_state, s->st_rng.ptr, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    return finish_path(s);
}

} // extern "C"

namespace pth {

std::vector<int> tile_owners(const pt_tile *tiles, size_t n_tiles, int n_scenes) {
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

int for_each_replica(int n, const std::function<int(int)> &fn) {
    std::vector<int> rcs(static_cast<size_t>(n), PT_OK);
    std::vector<std::string> errors(static_cast<size_t>(n));
    auto work = [&](int i) {
        rcs[static_cast<size_t>(i)] = fn(i);
        if(rcs[static_cast<size_t>(i)] != PT_OK) {
            errors[static_cast<size_t>(i)] = last_error(); // this thread's message
        }
    };
    std::vector<std::thread> threads;
    for(int i = 1; i < n; i++) {
        threads.emplace_back(work, i);
    }
    work(0);
    for(std::thread &t : threads) {
        t.join();
    }
    for(int i = 0; i < n; i++) {
        if(rcs[static_cast<size_t>(i)] != PT_OK) {
            return fail(rcs[static_cast<size_t>(i)], "scene " + std::to_string(i) + ": " + errors[static_cast<size_t>(i)]);
        }
    }
    return PT_OK;
}

void SharedProgress::step(int, int, void *shared) {
    SharedProgress *sh = static_cast<SharedProgress *>(shared);
    std::lock_guard<std::mutex> lock(sh->mutex);
    sh->completed++;
    sh->fn(sh->completed, sh->total, sh->user);
}

int copy_tile_rects(pt_scene *s, const std::vector<pt_tile> &tiles, const std::vector<size_t> &index, const uint8_t *skip, float *image, size_t width, bool to_device) {
    for(size_t k = 0; k < tiles.size(); k++) {
        if(skip != nullptr && skip[index[k]] != 0) {
            continue;
        }
        const pt_tile &t = tiles[k];
        const size_t at = static_cast<size_t>(t.y) * width + static_cast<size_t>(t.x);
        F4 *const dev = s->image.ptr + at;
        float *const host = image + at * 4;
        PT_HIP(hipMemcpy2DAsync(to_device ? static_cast<void *>(dev) : host, width * sizeof(F4), to_device ? static_cast<const void *>(host) : dev, width * sizeof(F4),
                                static_cast<size_t>(t.w) * sizeof(F4), static_cast<size_t>(t.h), to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, s->stream));
    }
    return PT_OK;
}

} // namespace pth

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
        PT_TRY(check_render_args(scenes[i], camera, options));
    }
    if(n_tiles == 0) {
        return PT_OK;
    }
    if(tiles == nullptr || out_image == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    const int32_t rows = views != nullptr ? views->rows(options) : options->image_height; // (a view batch: the stacked image)
    PT_TRY(check_tiles(tiles, n_tiles, options->image_width, rows, nullptr));
    // The multi-device form of doWorkParallel (src/worker.cpp:364-387): the tiles are dealt round-robin to the scenes (each a replica on its
    // own device; along the diagonals of a grid whose rows hold a multiple of n_scenes tiles, so that no device gets whole columns of the
    // frame -- cpupathtrace_amd/sharding.py uses the same rule), one host thread per scene drives its device, every device renders into its
    // own frame in HBM and only the rectangles of ITS tiles travel to the caller's image.  Engines are per pixel, so the image does not
    // depend on n_scenes.  progress calls are serialised and counted over all devices.
    const std::vector<int> owners = tile_owners(tiles, n_tiles, n_scenes);
    SharedProgress shared(progress, progress_user, 0, static_cast<int>(n_tiles));
    if(stats != nullptr) {
        std::memset(stats, 0, sizeof(*stats) * static_cast<size_t>(n_scenes));
    }
    const size_t width = static_cast<size_t>(options->image_width), pixels = width * static_cast<size_t>(rows);
    return for_each_replica(n_scenes, [&](int i) -> int {
        std::vector<pt_tile> mine;
        std::vector<size_t> mine_index;
        for(size_t k = 0; k < n_tiles; k++) {
            if(owners[k] == i) {
                mine.push_back(tiles[k]);
                mine_index.push_back(k);
            }
        }
        if(mine.empty()) {
            return PT_OK;
        }
        pt_scene *s = scenes[i];
        std::lock_guard<std::mutex> lock(s->render_mutex);
        PT_HIP(hipSetDevice(s->device));
        PT_HIP(s->image.ensure(pixels));
        PT_TRY(stop != nullptr ? copy_tile_rects(s, mine, mine_index, nullptr, out_image, width, true) : PT_OK);
        PT_TRY(render_tiles_impl(s, camera, options, mine.data(), mine.size(), base_seed, reinterpret_cast<float4 *>(s->image.ptr), stats != nullptr ? stats + i : nullptr,
                               shared.callback(), &shared, stop, views));
        PT_TRY(copy_tile_rects(s, mine, mine_index, nullptr, out_image, width, false));
        if(stop == nullptr) {
            return finish_path(s);
        }
        PT_TRY(finish_path(s, &tallies[i]));
        if(tile_done != nullptr) {
            // pixels of each tile not finished (render_tiles_impl set them to the tile's size, the kernel counted them down)
            std::vector<uint32_t> left(mine.size());
            PT_HIP(hipMemcpy(left.data(), s->tile_left.ptr, left.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for(size_t k = 0; k < mine.size(); k++) {
                tile_done[mine_index[k]] = left[k] == 0 ? 1 : 0;
            }
        }
        return PT_OK;
    });
}

// pt_render_tiles_device and pt_render_views_device behind their argument checks: a tile list, and the view set of a batch or null
static int render_tiles_device_impl(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const pt_tile *tiles, size_t n_tiles, uint64_t base_seed,
                                    const ViewSet *views, float *d_out_image, void *stream, pt_stats *stats) {
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    StreamOrder order;
    PT_TRY(order.begin(stream, s->stream));
    PT_TRY(render_tiles_impl(s, camera, options, tiles, n_tiles, base_seed, reinterpret_cast<float4 *>(d_out_image), stats, nullptr, nullptr, nullptr, views));
    PT_TRY(order.end());
    // These entry points do not wait for the device (the frame stays in HBM for the caller's stream).  With statistics they have waited
    // and checked already (run_path); PT_VERIFY=1 makes every call wait and check.
    return stats == nullptr && env_int("PT_VERIFY", 0) != 0 ? finish_path(s) : PT_OK;
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
    RenderStop stop(ctl, start);
    std::vector<StreamTally> tallies(n_scenes > 0 ? static_cast<size_t>(n_scenes) : 0U);
    PT_TRY(render_tiles_multi_impl(scenes, n_scenes, camera, options, tiles, n_tiles, base_seed, out_image, stats, progress, progress_user, &stop, ctl->tile_done,
                                           tallies.data()));
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
    PT_TRY(check_render_args(s, camera, options));
    if(stats != nullptr) {
        std::memset(stats, 0, sizeof(*stats));
    }
    if(n_tiles == 0) {
        return PT_OK;
    }
    if(tiles == nullptr || d_out_image == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    return render_tiles_device_impl(s, camera, options, tiles, n_tiles, base_seed, nullptr, d_out_image, stream, stats);
}

} // extern "C"

// ---- view batches (pt_render_views*): V cameras of one scene in one launch per replica ------------------------------------------------
// The views' frames are stacked into one image of V * H rows, view v = rows [v H, (v + 1) H), and the job is the tile list pt_job_tiles(W, H)
// of every view, moved down by v H, view after view.  The kernel finds a pixel's view from its row (pt_path.hip): its seed and camera ray
// are what pt_render_tiles(cameras[v], base_seeds[v]) gives the pixel at the local row, and the image store needs no change -- row-major
// W x (V H) is [V][H][W].  One view is that call itself.

namespace pth {

int prepare_views(const pt_camera_params *cameras, const uint64_t *base_seeds, int32_t n_views, const pt_options *options, std::vector<pt_tile> *tiles, ViewSet *views) {
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

} // namespace pth

extern "C" {

int pt_render_views(pt_scene *const *scenes, int n_scenes, const pt_camera_params *cameras, const uint64_t *base_seeds, int32_t n_views, const pt_options *options,
                    float *out_images, pt_stats *stats, pt_progress_fn progress, void *progress_user) {
    std::vector<pt_tile> tiles;
    ViewSet views;
    PT_TRY(prepare_views(cameras, base_seeds, n_views, options, &tiles, &views));
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
    PT_TRY(prepare_views(cameras, base_seeds, n_views, options, &tiles, &views));
    PT_TRY(check_render_args(s, cameras, options));
    if(stats != nullptr) {
        std::memset(stats, 0, sizeof(*stats));
    }
    if(d_out_images == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    return render_tiles_device_impl(s, cameras, options, tiles.data(), tiles.size(), base_seeds[0], n_views > 1 ? &views : nullptr, d_out_images, stream, stats);
}

} // extern "C"
