// pt_path.hip -- the hot path as ONE persistent kernel: per-pixel propagation loop (impl::getSample, src/worker.cpp:26-146), per-pixel
// estimator (processItem, src/worker.cpp:149-326) and closest-hit / shadow traversal of the reference's BVH
// (Scene::getIntersection, src/scene/scene.cpp:104-150,210-220).
//
// Every wavefront of the grid is an independent renderer.  It owns `rows` x 64 stream SLOTS (a slot = one processItem stream in
// progress: one engine, one path in flight), a private ring of rays in HBM and a few words per slot in LDS, and runs
//
//     loop:  retire finished walks (results -> LDS)
//            idle lanes?  queue has rays -> hand them out
//                         queue empty    -> SHADE every slot whose rays have all come back (one pass per row of 64 slots: coalesced
//                                           path state, exactly the reference's order of draws per stream), which appends new rays
//            TRACE: a burst of traversal steps for the 64 walks in the lanes
//
// until its slots have no stream left and the global stream counter is exhausted.  Nothing is ever synchronised between wavefronts
// (no grid barrier, no shared queue, no launch boundary): a ray that needs thousands of traversal steps keeps ONE lane busy and makes
// ONE stream miss a few shading passes, while the other 63 lanes and 255 slots go on -- in the two-kernel wavefront design of round 1
// every launch lasted as long as its slowest walk and the average wavefront was alive for 48 % of it (profiles/r01_pmc_*).
// Lanes are not tied to slots: a lane takes the next ray of the wave's queue whatever slot it belongs to, so the traversal runs on
// compacted, full wavefronts although the streams progress at different speeds.
//
// Traversal: the ordered recursion of impl::getChildIntersection restated as an iterative walk that visits exactly the leaves the
// recursion visits, in the same order:
//   * at an inner node both child boxes are tested (bounding_box.cpp:38-73); the nearer child is entered first, on equal entry
//     distances the RIGHT child is the nearer one (scene.cpp:120-121);
//   * a child is entered only if 0 <= entry < t_max (scene.cpp:124,137), where t_max is the smallest hit distance found so far -- in
//     the recursion t_max is threaded by value, but at every decision point it equals that global minimum, and the early return of
//     scene.cpp:129-132 is the same test (close hit < far entry  <=>  far entry >= t_max);
//   * the far child is parked on a per-lane stack TOGETHER with its entry distance and re-tested against the then-current t_max when
//     it is popped;
//   * a leaf reports Object::getIntersection unconditionally (scene.cpp:105-109); among non-negative hits the smallest wins and a
//     later-visited leaf wins ties (scene.cpp:141-146).
// Shadow rays (worker.cpp:84-86) only need "is there a visited leaf with 0 <= t < |to_light| - epsilon"; the walk stops at the first
// such leaf, which cannot change the answer.
// One traversal step serves inner nodes and leaves alike: every lane fetches the 64-byte record it stands on (a node's two child
// boxes, or a triangle) with the same four loads, so leaf tests cost no memory round trip of their own.  A step whose rare half (leaves,
// pops) runs requests records ONCE, behind it, for every lane: the rare half starts with no request of the common half in flight, and
// such a step waits for one record latency, not two (Tracer::step).
//
// gfx950 specifics: 64-wide ballots/popcounts for compaction, typed LDS/global address spaces (a pointer that may be either makes
// hipcc emit flat_load), per-lane traversal stack in LDS as [entry][lane] (conflict-free ds_read/write_b64) with an HBM spill area
// for unusually deep walks, LDS atomics for the per-slot completion words, no MFMA (there is no dense contraction on this path).
#include <type_traits>

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_shading.h"
#include "pt_trace.h"

using namespace ptd;

namespace {

// ---- the per-slot word in LDS -----------------------------------------------------------------------------------------------------------
// What the lanes that finish a slot's rays and the shading pass tell each other:
//   visibility of the last vertex's light samples (1 = unoccluded), set by the lanes that finish the shadow rays;
//   rays of the slot still in the queue or being walked;  PT_F_* flags of the slot.
// A lane that finishes a shadow ray adds (visibility bit) - (one ray) with ONE LDS atomic.
// Scene::sampleLights has no upper bound on the samples per vertex (every LightSource + min(2 + log10(E + 1), E) emitters, scene.cpp:226,231).
// Scenes with at most 8 of them -- every scene of the reference's programs -- use a 32-bit word that also holds which samples have a
// contribution waiting in S.nee (COMPACT: bits 0-7 visibility, 8-15 rays, 16-23 flags, 24-31 waiting); scenes with up to PT_MAX_NEE = 32
// use a 64-bit word (WIDE: bits 0-31 visibility, 32-39 rays, 40-47 flags) and keep the waiting mask with the slot's state in HBM
// (S.nee_mask: only the shading pass needs it).  The wide form costs the benchmark scene 5 % (one more load and store per slot and pass,
// 64-bit LDS traffic), which is why the compact one stays.
template<bool WIDE>
struct SlotWord {
    typedef uint32_t T;
    typedef uint32_t __attribute__((address_space(3))) *lds_ptr;
    static constexpr uint32_t j_mask = 7u;
    static PT_D uint32_t vis(T w) { return w & 0xffu; }
    static PT_D uint32_t pending(T w) { return (w >> 8) & 0xffu; }
    static PT_D uint32_t flags(T w) { return (w >> 16) & 0xffu; }
    static PT_D T one_ray() { return 0x100u; }
    static PT_D T make(uint32_t flags, uint32_t rays, uint32_t vis, uint32_t waiting) { return (waiting << 24) | (flags << 16) | (rays << 8) | vis; }
    static PT_D uint32_t waiting(T w, const PtSlots &, size_t) { return w >> 24; }
    static PT_D void keep_waiting(const PtSlots &, size_t, uint32_t) {}
};
template<>
struct SlotWord<true> {
    typedef unsigned long long T;
    typedef unsigned long long __attribute__((address_space(3))) *lds_ptr;
    static constexpr uint32_t j_mask = 31u;
    static PT_D uint32_t vis(T w) { return (uint32_t)w; }
    static PT_D uint32_t pending(T w) { return (uint32_t)(w >> 32) & 0xffu; }
    static PT_D uint32_t flags(T w) { return (uint32_t)(w >> 40) & 0xffu; }
    static PT_D T one_ray() { return 1ULL << 32; }
    static PT_D T make(uint32_t flags, uint32_t rays, uint32_t vis, uint32_t) { return ((T)flags << 40) | ((T)rays << 32) | (T)vis; }
    static PT_D uint32_t waiting(T, const PtSlots &S, size_t p) { return S.nee_mask[p]; }
    static PT_D void keep_waiting(const PtSlots &S, size_t p, uint32_t mask) { S.nee_mask[p] = mask; }
};

#define PT_F_VIEW_RAY 256u /* a view batch's camera ray is made at the end of the pass (shade_row); in the register only, never in the slot word */
#define PT_DEST_SLOT_MASK 0xffffu
#define PT_NO_SLOT 0xffffffffu
#define PT_DEST_J_SHIFT 16

// What a wavefront keeps about itself (everything wave-uniform).
struct WaveCtx {
    uint32_t q_head;   // index of the oldest queued ray inside the wave's ring
    uint32_t q_count;  // queued rays
    uint32_t n_dead;   // slots that will never get a stream again
    bool pool_empty;   // the global stream counter has run out
    uint32_t first_rows; // rows that have not taken their first streams yet (bit per row)
    uint32_t first_base; // the wave's own first streams: first_base + slot number
    uint32_t wave;       // number of the wavefront in the grid
};

// Stream i of a tile job: pixel i of the tiles laid end to end (pt_render_tiles)
PT_D void tile_stream(const PtStreams &T, uint32_t i, int4 &rect, uint64_t &rng, uint32_t &tile) {
    uint32_t lo = 0, hi = T.n_tiles;
    while(hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if(T.tile_offset[mid] <= i) {
            lo = mid;
        }
        else {
            hi = mid;
        }
    }
    const int4 t = T.tiles[lo];
    const uint32_t k = i - T.tile_offset[lo];
    const int32_t x = t.x + (int32_t)(k % (uint32_t)t.z), y = t.y + (int32_t)(k / (uint32_t)t.z);
    rect = make_int4(x, y, 1, 1);
    uint64_t base_seed = T.base_seed;
    int32_t seed_y = y;
    if(T.n_views > 1) {
        // a view batch: the pixel's own view and its row inside it (wave-uniform branch: n_views is a scalar of the launch)
        const uint32_t view = (uint32_t)y / T.view_height;
        base_seed = T.view_seed[view];
        seed_y = y - (int32_t)(view * T.view_height);
    }
    const uint64_t seed = pixel_seed(base_seed, x, seed_y);
    rng = seed ^ (~seed << 32); // RandomEngine(seed), base.h:26
    tile = lo;
}

// The small tables of the shading pass in LDS (PT_LDS_TABLE_MAX entries at most each; larger ones are read from global memory): the emitters'
// (EmisLds, pt_shading.h) and the materials
struct ShadeTables {
    EmisLds emis;
    lds_f4_cptr materials_l;
    bool emis_in_lds, materials_in_lds;
};

// dst[0 .. n) = src[0 .. n), one word at a time (a record is never held in registers whole)
PT_D void copy_words(void *dst, const void *src, uint32_t n) {
    uint32_t *d = static_cast<uint32_t *>(dst);
    const uint32_t *s = static_cast<const uint32_t *>(src);
#pragma unroll 1
    for(uint32_t i = 0; i < n; i++) {
        d[i] = s[i];
    }
}

// words of the candidates an estimator has closed (n_candidates counts on beyond the PT_MAX_CANDIDATES it keeps)
PT_D uint32_t closed_candidate_words(int32_t n_candidates) {
    return (uint32_t)(n_candidates < PT_MAX_CANDIDATES ? n_candidates : PT_MAX_CANDIDATES) * (uint32_t)(sizeof(PtCandidate) / 4);
}

// A resumable frame's stream leaves its slot (PtStreams::status): finished; or dropped by a stop request at a sample boundary, where a
// stream that has taken samples parks its engine, pixel, estimator and closed candidates in a record of park_out for a later launch.  A
// stream dropped before its first sample is untouched: it starts afresh from its seed next time, which gives the same bits.
PT_D void park_stream(const PtStreams &T, const PtSlots &S, uint32_t p, uint32_t stream, uint64_t rng, int32_t cursor, bool have_pixel) {
    uint32_t status = PT_STREAM_FINISHED;
    if(have_pixel) {
        status = PT_STREAM_UNTOUCHED;
        const PtEstimator *e = S.est + p;
        if(e->pixel_sample > 0 || cursor > 0) {
            const uint32_t k = atomicAdd(T.park_count, 1u);
            if(k < T.park_cap) { // (always: a launch parks at most one stream per slot -- per stream with yield_at -- and the host sizes park_out for that)
                PtParkRecord *rec = T.park_out + k;
                rec->stream = stream;
                rec->cursor = cursor;
                rec->rng[0] = (uint32_t)rng;
                rec->rng[1] = (uint32_t)(rng >> 32);
                copy_words(&rec->est, e, (uint32_t)(sizeof(PtEstimator) / 4));
                copy_words(rec->cand, S.cand + (size_t)p * PT_MAX_CANDIDATES, closed_candidate_words(e->n_candidates));
                status = PT_STREAM_PARKED + k;
            }
        }
    }
    T.status[stream] = status;
}

// Plane k of slot p (PtSlots): the scalar base plus a 32-bit byte offset, which becomes the saddr + voffset form of the load or store --
// no 64-bit address per plane lives in vector registers.
template<typename V>
PT_D V *slot_plane(const PtSlots &S, uint32_t k, uint32_t p) {
    return reinterpret_cast<V *>(reinterpret_cast<char *>(S.state) + (k * S.total + p) * (uint32_t)sizeof(float4));
}

// One shading pass over row `row` of the wave's slots: the state machine of one stream per lane.
//   * a slot without a stream takes the next one from the global counter (or dies when there is none left);
//   * a slot whose rays have all come back first adds the unoccluded light samples of its previous vertex to out_spectrum in the
//     reference's order (worker.cpp:76-103), then looks at the extension ray's hit: miss -> the sample is finished (estimator, next
//     sample or pixel); hit -> shade that vertex: emission (worker.cpp:62-64), Russian-roulette draw (:67-70), light sampling
//     (Scene::sampleLights, scene.cpp:222-289) with one shadow ray per light sample, BSDF sample (:117-131).
// A path that ends at a vertex (roulette) still has that vertex's shadow rays to wait for; where the estimator provably cannot stop
// at this sample, the NEXT sample's camera ray is drawn and traced together with them (PT_F_OVERLAP) -- the draws keep their order.
// The random draws of one stream are consumed strictly in the reference's order because a stream has at most one path in flight
// and every draw of a vertex (roulette, lights, BSDF) is made by the single invocation that shades the vertex.
// New rays go to the wave's ring: extension rays first, then the shadow rays light sample by light sample (ballot + prefix popcount
// give every lane its position; rays of one kind from neighbouring pixels end up in neighbouring lanes of the traversal).
template<bool WIDE>
PT_D void shade_row(const PtDevScene &sc, const PtDevCamera &cam, const PtDevOptions &opt, const PtSlots &S, const PtStreams &T, const PtLocalQueue &Q,
                    WaveCtx &ctx, uint32_t row, uint32_t ls_in, uint32_t lane, uint32_t slot_base, size_t queue_base, typename SlotWord<WIDE>::lds_ptr word_l, lds_u2_ptr hit_l,
                    float4 *__restrict__ image, PtDevCounters *counters, const ShadeTables &tb, bool stop, uint32_t &n_samples, uint32_t &n_vertices, uint32_t &n_shadow) {
    // (n_samples, n_vertices, n_shadow: the wavefront's counts, the same in every lane; stop: the host has asked the launch to stop (PtStreams::cancel),
    // a scalar read once per pass -- no stream is taken any more, and a stream that would start another sample is dropped instead)
    // the lane's slot of the wave: lane `lane` of row `row`, or -- in a compacted pass (see the kernel) -- the slot the list names; PT_NO_SLOT = none
    const bool have_slot = ls_in != PT_NO_SLOT;
    const uint32_t ls = have_slot ? ls_in : 0u;
    const uint32_t p = slot_base + ls;   // slot of the grid
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    const uint32_t n_light_samples = sc.n_lights + sc.n_object_samples;
    typedef SlotWord<WIDE> SW;
    const typename SW::T word = word_l[ls];
    uint32_t flags = SW::flags(word);
    const uint32_t vis_bits = SW::vis(word);
    bool ready = have_slot && !(flags & PT_F_DONE) && SW::pending(word) == 0;
    if(__ballot(ready) == 0ULL) {
        return;
    }

    // ---- slots without a stream: take the next one ------------------------------------------------------------------------------------
    {
        const bool want = ready && !(flags & PT_F_STREAM);
        const unsigned long long want_mask = __ballot(want);
        if(want_mask != 0ULL) {
            // A wavefront's FIRST streams are fixed (no race for the counter at kernel start: the same frame takes the same time twice) and
            // spread over the job.  The wavefront's slots are cut into pieces of `first_lanes` neighbouring slots (8: a quarter of a
            // tile's scanline); piece q of wavefront w starts on the chunk q * waves + w of as many streams, so the pieces of a wavefront
            // lie 1/32 of the first round apart and neighbouring wavefronts work on the same tiles; in a regular tile grid piece q is also
            // moved q steps sideways, so that a wavefront samples the frame's columns as well as its bands.  A wavefront costs what its
            // pixels cost, and the launch lasts as long as the most expensive wavefront: with 256 neighbouring pixels per wavefront the
            // benchmark frame runs at 294 Msamples/s, with four rows from four places (what the race for the counter used to produce)
            // at 393, with 32 pieces of 8 at 440.  Streams beyond the first round come from the global counter as the slots free up.
            uint32_t base = T.n;
            uint32_t mine;
            if((ctx.first_rows >> row) & 1u) {
                ctx.first_rows &= ~(1u << row);
                base = ctx.first_base + row * 64u;
                mine = base + lane;
                if(T.place != nullptr) {
                    // an explicit first round (cost-aware placement, pt_render.cpp): the table names the stream of every slot, or none
                    base = 0;
                    mine = T.place[ctx.first_base + ls];
                }
                else if(T.first_spread) {
                    // piece q of the wavefront (a row, or a part of one) starts on chunk q * waves + w of `first_lanes` streams
                    const uint32_t g = T.first_lanes, q = row * (64u / g) + lane / g;
                    uint32_t chunk = q * T.n_waves + ctx.wave;
                    if(T.tiles_per_row != 0) {
                        const uint32_t per_tile = T.chunks_per_tile * (64u / g), pieces = (T.first_total / T.n_waves) / g;
                        const uint32_t tile = chunk / per_tile, sub = chunk % per_tile;
                        const uint32_t step = T.tiles_per_row >= pieces ? T.tiles_per_row / pieces : 1u;
                        const uint32_t tx = (tile % T.tiles_per_row + q * T.first_shift * step) % T.tiles_per_row, ty = tile / T.tiles_per_row;
                        chunk = (ty * T.tiles_per_row + tx) * per_tile + sub;
                    }
                    base = 0; // (only compared with T.n below)
                    mine = chunk * g + lane % g;
                }
            }
            else {
                ctx.pool_empty = ctx.pool_empty || stop; // (a stop request leaves the rest of the pool unclaimed)
                if(!ctx.pool_empty) {
                    if(lane == 0) {
                        base = T.first_total + atomicAdd(T.next, (uint32_t)__popcll(want_mask));
                    }
                    base = __builtin_amdgcn_readfirstlane(base);
                }
                mine = base + (uint32_t)__popcll(want_mask & lt);
                if(base >= T.n || base + (uint32_t)__popcll(want_mask) > T.n) {
                    ctx.pool_empty = true;
                }
            }
            const bool got = want && base < T.n && mine < T.n;
            if(got) {
                int4 rc;
                uint64_t r;
                uint32_t tile = 0;
                uint32_t park = PT_NO_PARK;
                int32_t cursor0 = 0;
                if(T.rect != nullptr) {
                    rc = T.rect[mine];
                    r = T.rng[mine];
                }
                else {
                    if(T.todo != nullptr) {
                        // a resumable frame: the launch's stream `mine` is the frame's stream todo[mine], parked or fresh
                        const uint2 entry = T.todo[mine];
                        mine = entry.x;
                        park = entry.y;
                    }
                    tile_stream(T, mine, rc, r, tile);
                }
                flags = PT_F_STREAM;
                if(park != PT_NO_PARK) {
                    // a parked stream goes on at the sample boundary where it was dropped: engine, pixel, estimator and closed
                    // candidates come from its record, and the start of the next sample does not reset the estimator (PT_F_PIXEL)
                    const PtParkRecord *rec = T.park_in + park;
                    r = (uint64_t)rec->rng[0] | ((uint64_t)rec->rng[1] << 32);
                    cursor0 = rec->cursor;
                    copy_words(S.est + p, &rec->est, (uint32_t)(sizeof(PtEstimator) / 4));
                    copy_words(S.cand + (size_t)p * PT_MAX_CANDIDATES, rec->cand, closed_candidate_words(rec->est.n_candidates));
                    flags = PT_F_STREAM | PT_F_PIXEL | (estimator_safe_to_overlap(S.est[p], opt) ? PT_F_SAFE : 0u);
                }
                *slot_plane<int4>(S, PT_PLANE_RECT, p) = rc;
                *slot_plane<uint4>(S, PT_PLANE_ENGINE, p) = make_uint4((uint32_t)r, (uint32_t)(r >> 32), (uint32_t)cursor0, mine);
                if(T.cost != nullptr) {
                    __hip_atomic_store(&S.cost[p], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            else if(want) {
                flags = PT_F_DONE;
                ready = false;
                word_l[ls] = SW::make(PT_F_DONE, 0u, 0u, 0u);
            }
            ctx.n_dead += (uint32_t)__popcll(__ballot(want && !got));
        }
    }
    const bool alive = ready;
    uint32_t lane_samples = 0; // samples this lane completes here (0, 1 or 2): added to the wavefront's count at the end

    // ---- phase A: consume the results of the rays that came back -----------------------------------------------------------------------
    uint64_t rng = 0;
    C4 out = c4(0, 0, 0, 0), spectrum = c4(1, 1, 1, 1);
    V3 ro = v3(0, 0, 0), rd = v3(0, 0, 1);
    float contribution_unweighted = 1.0f;
    double divisor = 1.0, bounce_pd = 1.0;
    int path_length = 0;
    bool shade_vertex = false; // the extension ray hit something
    bool start_sample = false; // generate a camera ray
    float hit_t = -1.0f;
    uint32_t hit_ref = PT_REF_NONE;
    int4 rect = make_int4(0, 0, 0, 0);
    int32_t cursor = 0;
    uint32_t stream = 0;
    bool stream_finished = false;
    bool stream_abandoned = false; // dropped at a sample boundary after a stop request: no pixel, no engine state, no cost, no tile count

    if(alive) {
        const uint4 engine = *slot_plane<uint4>(S, PT_PLANE_ENGINE, p);
        rng = (uint64_t)engine.x | ((uint64_t)engine.y << 32);
        cursor = (int32_t)engine.z;
        stream = engine.w;
        rect = *slot_plane<int4>(S, PT_PLANE_RECT, p);
        if(flags & PT_F_IN_FLIGHT) {
            // Everything the slot may need is requested here, in one batch (one memory round trip instead of one per use): the path
            // state, and -- a single word, to bring the line into the caches -- the shading record of the triangle that was hit, which
            // is the one access of this pass that usually comes from HBM.
            const float4 out4 = *slot_plane<float4>(S, PT_PLANE_OUT, p);
            uint32_t mask = SW::waiting(word, S, p);
            // the first two light samples (most scenes have no more) are fetched with the batch, the others one by one below
            const uint32_t lit = mask & vis_bits;
            float4 nee0 = make_float4(0, 0, 0, 0), nee1 = make_float4(0, 0, 0, 0);
            if(lit & 1u) {
                nee0 = S.nee[p];
            }
            if(lit & 2u) {
                nee1 = S.nee[S.total + p];
            }
            const float4 o4 = *slot_plane<float4>(S, PT_PLANE_RAY_O, p), d4 = *slot_plane<float4>(S, PT_PLANE_RAY_D, p);
            const float4 spectrum4 = *slot_plane<float4>(S, PT_PLANE_SPECTRUM, p);
            const double2 pd_in = *slot_plane<double2>(S, PT_PLANE_PD, p);
            uint32_t warm = 0;
            if(flags & PT_F_HAS_EXT) {
                const u2v h = hit_l[ls];
                hit_t = __uint_as_float(h.x);
                hit_ref = h.y;
                if(!(hit_t < 0.0f) && !(hit_ref & PT_REF_SPHERE)) {
                    warm = *reinterpret_cast<const uint32_t *>(sc.tri_shade + 8 * (size_t)(hit_ref & PT_REF_INDEX));
                }
            }
            out = c4(out4);
            // shadow rays of the previous vertex, in light order (worker.cpp:76-103)
            if(lit & 1u) {
                out = out + c4(nee0);
            }
            if(lit & 2u) {
                out = out + c4(nee1);
            }
            mask >>= 2;
            for(uint32_t j = 2; mask != 0; j++, mask >>= 1) {
                if((mask & 1u) && ((vis_bits >> j) & 1u)) {
                    out = out + c4(S.nee[(size_t)j * S.total + p]);
                }
            }
            asm volatile("" ::"v"(warm)); // (the word itself is not used)
            if(flags & PT_F_OVERLAP) {
                // the previous sample is complete now (worker.cpp:141-145, 196-237); it was collected (it had a vertex), it is
                // not the pixel's last sample and the estimator cannot accept at it (see estimator_safe_to_overlap)
                PtEstimator e = S.est[p];
                out.a = 1.0f;
                (void)estimator_add(e, S.cand + (size_t)p * PT_MAX_CANDIDATES, opt, out);
                e.pixel_sample++;
                lane_samples++;
                S.est[p] = e;
                flags &= ~(PT_F_OVERLAP | PT_F_COLLECTED | PT_F_SAFE);
                if(estimator_safe_to_overlap(e, opt)) {
                    flags |= PT_F_SAFE;
                }
                out = c4(0, 0, 0, 0);
            }
            bool finished = true;
            if((flags & PT_F_HAS_EXT) && !(hit_t < 0.0f)) {
                finished = false;
                shade_vertex = true;
            }
            if(finished) {
                // getSample returns (worker.cpp:141-145); run the estimator
                PtEstimator e = S.est[p];
                PtCandidate *cand = S.cand + (size_t)p * PT_MAX_CANDIDATES;
                bool accepted = false;
                if(flags & PT_F_COLLECTED) {
                    out.a = 1.0f;
                    accepted = estimator_add(e, cand, opt, out);
                }
                e.pixel_sample++;
                lane_samples++;
                if(accepted || e.pixel_sample >= opt.max_sample_count) {
                    // pixel finished (worker.cpp:263-319)
                    const C4 value = estimator_finish(e, cand, opt, accepted);
                    const int32_t px = rect.x + cursor % rect.z, py = rect.y + cursor / rect.z;
                    image[(size_t)py * opt.image_width + px] = f4(value);
                    cursor++;
                    flags &= ~PT_F_PIXEL;
                }
                S.est[p] = e;
                flags &= ~(PT_F_IN_FLIGHT | PT_F_HAS_EXT | PT_F_COLLECTED | PT_F_SAFE);
                if((flags & PT_F_PIXEL) && estimator_safe_to_overlap(e, opt)) {
                    flags |= PT_F_SAFE; // for the pixel's next sample, which starts below
                }
                start_sample = true;
            }
            else {
                ro = v3(o4.x, o4.y, o4.z);
                rd = v3(d4.x, d4.y, d4.z);
                contribution_unweighted = o4.w;
                spectrum = c4(spectrum4);
                divisor = pd_in.x;
                bounce_pd = pd_in.y;
                path_length = __float_as_int(d4.w);
            }
        }
        else {
            start_sample = true;
        }
    }

    // ---- start the next sample / pixel ------------------------------------------------------------------------------------
    bool emit_ext = false;
    Ray ext;
    ext.o = v3(0, 0, 0);
    ext.d = v3(0, 0, 1);
    // camera ray through pixel `cur` of the stream's rectangle (worker.cpp:168-170, camera.cpp:78-113)
    auto shoot_camera = [&](const int4 rc, int32_t cur) {
        const int32_t px = rc.x + cur % rc.z, py = rc.y + cur / rc.z;
        const float one_half = 1.0f / 2.0f;
        const float x_camera = 2 * (((float)px + one_half) / (float)opt.image_width - one_half);
        float y_camera = 2 * (((float)py + one_half) / (float)opt.image_height - one_half);
        y_camera = -y_camera;
        return camera_shoot(cam, x_camera, y_camera, opt.pixel_width, opt.pixel_height, rng);
    };
    // In a view batch (T.n_views > 1: a scalar, so every test of it is wave-uniform) a camera ray is not made where it is called for but once,
    // at the end of the pass: the camera differs from lane to lane there (lanes of one row of slots may hold pixels of different
    // views), and its fields are vector registers that the start of a sample has no room for.  The order of draws is unchanged: a lane that
    // starts a sample makes no other draw in the pass, and the overlapped camera ray is the last draw of a vertex.
    // (Which lanes want one is a flag bit of the register `flags`, never stored: a lane mask of its own, live across the light samples, costs spills.)
    const bool batch = T.n_views > 1;
    if(start_sample) {
        bool have_pixel = false;
        while(cursor < rect.z * rect.w) {
            if(!(flags & PT_F_PIXEL)) {
                PtEstimator e;
                estimator_reset(e, opt);
                S.est[p] = e;
                flags = (flags | PT_F_PIXEL) & ~PT_F_SAFE;
                if(estimator_safe_to_overlap(e, opt)) {
                    flags |= PT_F_SAFE;
                }
                if(opt.max_sample_count <= 0) {
                    // no sample at all: the pixel stays (0, 0, 0, 0) (worker.cpp:193,263-265)
                    const int32_t px = rect.x + cursor % rect.z, py = rect.y + cursor / rect.z;
                    image[(size_t)py * opt.image_width + px] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    cursor++;
                    flags &= ~PT_F_PIXEL;
                    continue;
                }
            }
            have_pixel = true;
            break;
        }
        // (a pass of a progressive frame: the pixel has the pass's sample count -- one word of the estimator against a scalar)
        const bool yield = T.yield_at != 0 && have_pixel && S.est[p].pixel_sample >= T.yield_at;
        if(!have_pixel || stop || yield) {
            // the stream has rendered its whole rectangle: hand the engine back and free the slot (it takes a new stream in the next pass).
            // After a stop request a stream that has a pixel left is dropped here instead, between two samples, with no ray in flight (a
            // slot is only shaded once all its rays are back): every pixel it finished is exact, its current pixel is never written, and
            // its slot is freed in the same way -- since the pool is closed, it dies in its next pass.  A stream that yields (PtStreams::yield_at)
            // leaves in the same way without a stop: the pool is open then, and its slot takes the next stream in its next pass.
            stream_finished = !have_pixel;
            stream_abandoned = have_pixel;
            if(T.status != nullptr) {
                park_stream(T, S, p, stream, rng, cursor, have_pixel);
            }
            flags = 0;
        }
        else {
            if(batch) {
                flags |= PT_F_VIEW_RAY;
                ext.o = v3(0, 0, 0); // (a constant: what ext held must not stay live until the ray is made)
                ext.d = v3(0, 0, 1);
            }
            else {
                ext = shoot_camera(rect, cursor);
            }
            emit_ext = true;
            out = c4(0, 0, 0, 0);
            spectrum = c4(1, 1, 1, 1);
            contribution_unweighted = 1.0f;
            divisor = 1.0;
            bounce_pd = 1.0;
            path_length = 0;
            flags |= PT_F_IN_FLIGHT | PT_F_HAS_EXT;
        }
    }
    {
        const unsigned long long fin_mask = __ballot(stream_finished);
        if(fin_mask != 0ULL) {
            if(stream_finished) {
                const uint32_t si = stream;
                if(T.rng != nullptr) {
                    T.rng[si] = rng;
                }
                if(T.cost != nullptr) {
                    T.cost[si] = __hip_atomic_load(&S.cost[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (written by atomics of this wavefront's lanes: read it where they landed)
                }
                if(T.tile_left != nullptr) {
                    // progress: the last pixel of a tile reports the tile to the host (processJob's callback, worker.cpp:354-360)
                    int4 rc_unused;
                    uint64_t r_unused;
                    uint32_t tile = 0;
                    tile_stream(T, si, rc_unused, r_unused, tile);
                    if(atomicSub(&T.tile_left[tile], 1u) == 1u) {
                        __hip_atomic_fetch_add(T.tiles_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                }
            }
            if(lane == 0) {
                atomicAdd(&counters->streams_done, (unsigned long long)__popcll(fin_mask));
            }
        }
        if(stop || T.yield_at != 0) {
            const unsigned long long drop_mask = __ballot(stream_abandoned);
            if(lane == 0 && drop_mask != 0ULL) {
                atomicAdd(&counters->streams_abandoned, (unsigned long long)__popcll(drop_mask));
            }
        }
    }

    // ---- vertex, part 1: everything up to the Russian-roulette draw (worker.cpp:50-70) ---------------------------------------
    V3 pos = v3(0, 0, 0), n = v3(0, 1, 0);
    Material mat;
    mat.bsdf = 0;
    bool do_bounce = false;
    float bounce_probability = 1.0f;
    bool want_nee = false;
    bool safe_overlap = false;
    if(shade_vertex) {
        path_length++;
        flags |= PT_F_COLLECTED;
        pos = ro + rd * hit_t;
        uint32_t material_index;
        n = object_normal(sc, hit_ref, pos, material_index);
        mat = tb.materials_in_lds ? material_load(tb.materials_l, material_index) : material_load(sc.materials, material_index);

        out = out + (spectrum * mat.emission) / (float)(divisor * bounce_pd);

        bounce_probability = path_length <= 4 ? 1.0f : 0.1f + 0.1f * fmin_std(contribution_unweighted * get_contribution(spectrum), 1.0f);
        do_bounce = rng_uniform01(rng) < bounce_probability;
        // BSDF::getSpectrum(..., synthetic = true) returns p = 0 for glass and mirror: their light samples never
        // contribute (worker.cpp:92), so no shadow ray is needed -- the light-sampling draws are still consumed below.
        want_nee = mat.bsdf == 0 && n_light_samples > 0;
        // (decided when the sample started, estimator_safe_to_overlap; after a stop request no sample is overlapped, so that the next
        // boundary -- where the stream is dropped -- comes as soon as this path ends)
        safe_overlap = (flags & PT_F_SAFE) != 0 && !stop;
        // an extension ray: the bounce (may still be cancelled by the 1E-20 guards, worker.cpp:112,134) or the next sample's camera ray
        emit_ext = do_bounce || safe_overlap;
    }

    // ---- positions in the wave's ring: extension rays first (the long walks start first) -------------------------------------------------
    uint32_t tail = ctx.q_head + ctx.q_count; // may be >= cap: wrapped per entry below
    const unsigned long long ext_mask = __ballot(emit_ext);
    const uint32_t ext_pos = tail + (uint32_t)__popcll(ext_mask & lt);
    tail += (uint32_t)__popcll(ext_mask);
    ctx.q_count += (uint32_t)__popcll(ext_mask);
    n_shadow -= (uint32_t)__popcll(ext_mask); // (the kernel adds what the pass queued: what is left are the shadow rays)
    auto ring = [&](uint32_t i) -> size_t { return queue_base + (i >= Q.cap ? i - Q.cap : i); };

    // ---- vertex, part 2: light sampling, shadow rays (worker.cpp:73-103) -------------------------------------------------------------------
    uint32_t nee_out_mask = 0;
    uint32_t vis_init = 0;
    uint32_t n_rays = 0;
    const float epsilon = opt.epsilon;
    for(uint32_t j = 0; j < n_light_samples; j++) { // wave-uniform trip count
        bool need_ray = false;
        float4 so = make_float4(0, 0, 0, 0), sd = make_float4(0, 0, 0, 0);
        if(shade_vertex) {
            V3 light_pos;
            C4 light_spectrum;
            float lpd;
            bool valid;
            if(j < sc.n_lights) {
                // PointLightSource: its position, its spectrum, pd = 1 (light.cpp:35-41)
                const float4 lp = sc.lights[2 * j];
                light_pos = v3(lp.x, lp.y, lp.z);
                light_spectrum = c4(sc.lights[2 * j + 1]);
                lpd = 1.0f;
                valid = true;
            }
            else {
                valid = tb.emis_in_lds ? sample_emissive(sc, tb.emis, pos, rng, light_pos, light_spectrum, lpd)
                                       : sample_emissive(sc, EmisGlobal{sc}, pos, rng, light_pos, light_spectrum, lpd);
            }
            if(valid && want_nee) {
                const V3 to_light = light_pos - pos;
                const V3 light_dir = normalize(to_light);
                float shading_factor, shadow_ray_pd;
                const C4 base_spectrum = bsdf_spectrum(mat, rd, light_dir, n, light_spectrum, true, shading_factor, shadow_ray_pd);
                if(shadow_ray_pd > 0.0f) {
                    const C4 combined = (base_spectrum * shading_factor) * spectrum;
                    const C4 weighed = combined / (float)(divisor * bounce_pd * lpd * shadow_ray_pd);
                    // adding +-0 never changes out_spectrum (which is never -0), so such a sample needs no ray
                    if(!(weighed.r == 0.0f && weighed.g == 0.0f && weighed.b == 0.0f)) {
                        S.nee[(size_t)j * S.total + p] = f4(weighed);
                        nee_out_mask |= 1u << j;
                        const float threshold = len(to_light) - epsilon;
                        if(threshold <= 0.0f) {
                            // light_t < 0 || light_t >= threshold holds for every light_t
                            vis_init |= 1u << j;
                        }
                        else {
                            need_ray = true;
                            const V3 o2 = pos + light_dir * epsilon;
                            so = make_float4(o2.x, o2.y, o2.z, threshold);
                            sd = make_float4(light_dir.x, light_dir.y, light_dir.z, __uint_as_float(PT_DEST_SHADOW | (j << PT_DEST_J_SHIFT) | ls));
                        }
                    }
                }
            }
        }
        const unsigned long long ray_mask = __ballot(need_ray);
        if(ray_mask != 0ULL) {
            if(need_ray) {
                const size_t at = ring(tail + (uint32_t)__popcll(ray_mask & lt));
                Q.ray_o[at] = so;
                Q.ray_d[at] = sd;
                n_rays++;
            }
            tail += (uint32_t)__popcll(ray_mask);
            ctx.q_count += (uint32_t)__popcll(ray_mask);
        }
    }

    // ---- vertex, part 3: the bounce (worker.cpp:105-138) ---------------------------------------------------------------------------------
    if(shade_vertex) {
        bool cancel_ext = false;
        if(!do_bounce) {
            // worker.cpp:106-109: the path ends here
        }
        else {
            bounce_pd *= bounce_probability;
            if(bounce_pd <= 1E-20) {
                cancel_ext = true;
            }
            else {
                float ray_factor, ray_pd;
                const Ray next_ray = bsdf_propagate(mat, rd, pos, n, epsilon, rng, ray_factor, ray_pd);
                divisor *= ray_pd;
                divisor /= ray_factor;
                contribution_unweighted *= ray_factor;
                float shading_factor, shading_pd;
                const C4 shaded = bsdf_spectrum(mat, rd, next_ray.d, n, spectrum, false, shading_factor, shading_pd);
                divisor *= shading_pd;
                divisor /= shading_factor;
                contribution_unweighted *= shading_factor;
                spectrum = shaded;
                if(divisor <= 1E-20) {
                    cancel_ext = true;
                }
                else {
                    ext = next_ray;
                }
            }
        }
        const bool path_ends = !do_bounce || cancel_ext;
        if(path_ends && safe_overlap) {
            // start the next sample of this pixel now; this sample is finished by the next pass over the slot (PT_F_OVERLAP)
            if(batch) {
                flags |= PT_F_VIEW_RAY;
                ext.o = v3(0, 0, 0); // (a constant: what ext held must not stay live until the ray is made)
                ext.d = v3(0, 0, 1);
            }
            else {
                ext = shoot_camera(rect, cursor);
            }
            spectrum = c4(1, 1, 1, 1);
            contribution_unweighted = 1.0f;
            divisor = 1.0;
            bounce_pd = 1.0;
            path_length = 0;
            flags |= PT_F_OVERLAP;
        }
        else if(path_ends && emit_ext) {
            // the reserved position stays a hole (a bounce cancelled by the 1E-20 guards: rare)
            Q.ray_d[ring(ext_pos)] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(PT_DEST_NULL));
            emit_ext = false;
        }
        if(emit_ext) {
            flags |= PT_F_HAS_EXT;
        }
        else {
            flags &= ~PT_F_HAS_EXT;
        }
    }

    // ---- a view batch's camera rays: the pixel's view is its row / H, its camera that view's record of the table ------------------------------
    if(flags & PT_F_VIEW_RAY) {
        flags &= ~PT_F_VIEW_RAY;
        const int32_t px = rect.x + cursor % rect.z, row = rect.y + cursor / rect.z;
        const uint32_t view = (uint32_t)row / (uint32_t)opt.image_height;
        const int32_t py = row - (int32_t)(view * (uint32_t)opt.image_height);
        const float one_half = 1.0f / 2.0f;
        const float x_camera = 2 * (((float)px + one_half) / (float)opt.image_width - one_half);
        float y_camera = 2 * (((float)py + one_half) / (float)opt.image_height - one_half);
        y_camera = -y_camera;
        ext = camera_shoot_lane(T.views[view].cam, x_camera, y_camera, opt.pixel_width, opt.pixel_height, rng);
    }

    // ---- write the extension ray and the path state ------------------------------------------------------------------------------
    if(emit_ext) {
        const size_t at = ring(ext_pos);
        Q.ray_o[at] = make_float4(ext.o.x, ext.o.y, ext.o.z, 0.0f);
        Q.ray_d[at] = make_float4(ext.d.x, ext.d.y, ext.d.z, __uint_as_float(ls));
        n_rays++;
    }
    if(alive) {
        word_l[ls] = SW::make(flags, n_rays, vis_init, nee_out_mask);
        SW::keep_waiting(S, p, nee_out_mask);
        // (rng and cursor: the stream index in .w stays as it is)
        *slot_plane<uint3>(S, PT_PLANE_ENGINE, p) = make_uint3((uint32_t)rng, (uint32_t)(rng >> 32), (uint32_t)cursor);
        if(flags & PT_F_IN_FLIGHT) {
            *slot_plane<float4>(S, PT_PLANE_RAY_O, p) = make_float4(ext.o.x, ext.o.y, ext.o.z, contribution_unweighted);
            *slot_plane<float4>(S, PT_PLANE_RAY_D, p) = make_float4(ext.d.x, ext.d.y, ext.d.z, __int_as_float(path_length));
            *slot_plane<float4>(S, PT_PLANE_SPECTRUM, p) = f4(spectrum);
            *slot_plane<float4>(S, PT_PLANE_OUT, p) = f4(out);
            *slot_plane<double2>(S, PT_PLANE_PD, p) = make_double2(divisor, bounce_pd);
        }
    }
    // (wavefront totals: per-lane counters would be two more registers live across every pass)
    n_samples += (uint32_t)__popcll(__ballot(lane_samples & 1u)) + 2u * (uint32_t)__popcll(__ballot((lane_samples & 2u) != 0u));
    n_vertices += (uint32_t)__popcll(__ballot(shade_vertex));
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------------------

#ifndef PT_COST_LDS_BYTES
#define PT_COST_LDS_BYTES 1024 /* one word per lane: the wave step at which its walk began (stream cost diagnostics); 0 in builds that need the LDS */
#endif
#ifndef PT_PATH_WAVES
#define PT_PATH_WAVES 4 /* 128 VGPRs: the traversal loop has no spills there; three waves per SIMD hide less of the node-fetch latency (profiles/) */
#endif

// The lane's number, computed afresh where it is asked for: the asm is opaque, so the compiler cannot reuse a lane number (or anything
// computed from it) from before a shading pass and carry it through the pass in a register.
PT_D uint32_t lane_afresh() {
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

template<bool WIDE, bool IN_LDS, int STACK_LDS>
__global__ __launch_bounds__(256, PT_PATH_WAVES) void pt_path_kernel(const PtPathArgs *__restrict__ args) {
    typedef SlotWord<WIDE> SW;
    // The argument block is read-only for the whole launch: it is addressed as CONSTANT memory (scalar loads; and pointers loaded from
    // constant memory are known to be global ones, so everything reached through them stays global_load / global_store).
    const args_c4 A4 = (args_c4)args;
    const PtPathArgs *A = (const PtPathArgs *)A4;
    // what the traversal loop needs, read once
    const int rows = A->rows, slots_per_wave = A->slots_per_wave, refill_idle = A->refill_idle, min_ready = A->min_ready, burst_steps = A->burst_steps,
              leaf_min = A->leaf_min, ready_shift = A->ready_shift, pass_q_low = A->early_ready > 0 ? A->pass_q_low : 0, early_ready = A->early_ready;
    // diagnostic (PT_DEBUG_LANES): only the first `debug_lanes` lanes of a wavefront take rays -- throughput against walks per step with everything else equal
    const unsigned long long lane_cap = A->debug_lanes >= 64 ? ~0ULL : ((1ULL << A->debug_lanes) - 1ULL);
    PtLocalQueue Q = A->Q;
    // (the ring as the traversal loop reads it: typed global, so the window's reloads are global_load, not flat_load -- which would also count
    // in lgkmcnt, where the next step's stack read waits)
    const glb_f4_cptr ring_o = (glb_f4_cptr)reinterpret_cast<const f4v *>(Q.ray_o), ring_d = (glb_f4_cptr)reinterpret_cast<const f4v *>(Q.ray_d);
    RootBox root;
    root.ref = A->sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = A->sc.root_lo[k];
        root.hi[k] = A->sc.root_hi[k];
    }
    extern __shared__ __align__(16) unsigned char lds_raw[];
    // LDS of the workgroup: traversal stacks [STACK_LDS][256] | hit records [4 waves][rows * 64] | slot words [4 waves][rows * 64] |
    // emitter and material tables (PT_LDS_TABLE_BYTES) | start step of every lane's walk | (small scenes) the whole tree and all triangle records
    const int tid = threadIdx.x;
    uint32_t lane = (uint32_t)tid & 63u;
    // (read from the first lane: the compiler does not know that tid >> 6 is the same in every lane, and would keep the wavefront's
    // number and everything computed from it -- the slot, ring and LDS bases -- in vector registers that the shading pass spills)
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane((uint32_t)tid >> 6);
    const uint32_t wave = blockIdx.x * 4u + wave_in_block;
    const uint32_t n_slots = (uint32_t)rows * 64u;
    unsigned char *at = lds_raw;
    const lds_u2_ptr stack_base = (lds_u2_ptr)reinterpret_cast<uint2 *>(at) + wave_in_block * 64u;
    at += (size_t)STACK_LDS * 256 * sizeof(uint2);
    lds_u2_ptr hit_l = (lds_u2_ptr)reinterpret_cast<uint2 *>(at) + wave_in_block * n_slots;
    at += (size_t)4 * n_slots * sizeof(uint2);
    typename SW::lds_ptr word_l = (typename SW::lds_ptr)reinterpret_cast<typename SW::T *>(at) + wave_in_block * n_slots;
    at += (size_t)4 * n_slots * sizeof(typename SW::T);
    float *cdf_l = reinterpret_cast<float *>(at);
    at += (size_t)PT_LDS_TABLE_MAX * sizeof(float);
    float4 *emis_l = reinterpret_cast<float4 *>(at);
    at += (size_t)PT_LDS_TABLE_MAX * 4 * sizeof(float4);
    float4 *light_l = reinterpret_cast<float4 *>(at);
    at += (size_t)PT_LDS_TABLE_MAX * 6 * sizeof(float4);
    float4 *materials_l = reinterpret_cast<float4 *>(at);
    at += (size_t)PT_LDS_TABLE_MAX * 4 * sizeof(float4);
    typedef uint32_t __attribute__((address_space(3))) *lds_u32_ptr;
    const lds_u32_ptr born_base = (lds_u32_ptr)reinterpret_cast<uint32_t *>(at) + wave_in_block * 64u;
    lds_u32_ptr born_l = born_base + lane; // wave step at which the lane's walk began
    // (the same kilobyte holds the list of ready slots of a compacted shading pass, one byte per slot of up to four rows, when the cost diagnostics are off)
    typedef unsigned char __attribute__((address_space(3))) *lds_u8_ptr;
    lds_u8_ptr list_l = (lds_u8_ptr)reinterpret_cast<unsigned char *>(at) + wave_in_block * 256u;
    at += (size_t)PT_COST_LDS_BYTES;
    float4 *lds_recs = reinterpret_cast<float4 *>(at); // (small scenes) every record, in the order of `recs`
    const bool cost_on = PT_COST_LDS_BYTES != 0 && A->T.cost != nullptr;
    uint32_t *const slot_cost = A->S.cost;

    ShadeTables tb;
    tb.emis.cdf_l = (const float __attribute__((address_space(3))) *)cdf_l;
    tb.emis.rec_l = (lds_f4_cptr)emis_l;
    tb.emis.light_l = (lds_f4_cptr)light_l;
    tb.materials_l = (lds_f4_cptr)materials_l;
    {
        const uint32_t n_emis = A->sc.n_emis, n_materials = A->sc.n_materials;
        tb.emis_in_lds = n_emis > 0 && n_emis <= PT_LDS_TABLE_MAX;
        tb.materials_in_lds = n_materials > 0 && n_materials <= PT_LDS_TABLE_MAX;
        if(tb.emis_in_lds) {
            const float4 *src_emis = A->sc.emis, *src_shade = A->sc.tri_shade;
            const float *src_cdf = A->sc.emis_cdf;
            for(uint32_t i = tid; i < n_emis; i += 256) {
                cdf_l[i] = src_cdf[i];
            }
            for(uint32_t i = tid; i < 4 * n_emis; i += 256) {
                emis_l[i] = src_emis[i];
            }
            for(uint32_t i = tid; i < 6 * n_emis; i += 256) {
                const uint32_t ref = __float_as_uint(src_emis[4 * (i / 6) + 2].y);
                light_l[i] = (ref & PT_REF_SPHERE) ? make_float4(0, 0, 0, 0) : src_shade[8 * (size_t)(ref & PT_REF_INDEX) + i % 6];
            }
        }
        if(tb.materials_in_lds) {
            const float4 *src_materials = A->sc.materials;
            for(uint32_t i = tid; i < 4 * n_materials; i += 256) {
                materials_l[i] = src_materials[i];
            }
        }
    }

    if(IN_LDS) {
        const uint32_t n_lds_quads = 4u * (A->sc.pair_base + A->sc.n_pairs);
        const float4 *src_recs = A->sc.recs;
        for(uint32_t i = tid; i < n_lds_quads; i += 256) {
            lds_recs[i] = src_recs[i];
        }
    }
    for(uint32_t i = lane; i < n_slots; i += 64) {
        // no stream, nothing pending: ready to take a stream.  (A small job uses only the first slots of every wavefront: its streams are
        // spread over all the wavefronts the chip holds, because a stream's samples are sequential and only more wavefronts shorten the chain.)
        word_l[i] = i < (uint32_t)slots_per_wave ? (typename SW::T)0 : SW::make(PT_F_DONE, 0u, 0u, 0u);
    }
    __syncthreads(); // the only barrier: from here on the four wavefronts of the workgroup never wait for each other

    Tracer<STACK_LDS, IN_LDS, true> tr;
    if(IN_LDS) {
        tr.recs = (typename RecPtr<IN_LDS>::type)(lds_f4_cptr)lds_recs;
    }
    else {
        tr.recs = (typename RecPtr<IN_LDS>::type)(glb_f4_cptr)A->sc.recs;
    }
    // What depends on the lane number is derived again on every entry into the traversal loop (from a fresh lane number and the argument
    // block) instead of living through a shading pass in vector registers.  (Bound only after a pass, the values would merge with the
    // ones bound before it, and the compiler kept that merged value in scratch -- reloaded by every refill of the traversal loop.)
    auto bind_lane = [&](const PtPathArgs *B, uint32_t l) {
        lane = l;
        tr.stack_l = stack_base + l;
        tr.my_spill = (glb_u2_ptr)(B->spill + ((size_t)wave * 64 + l) * B->spill_depth);
        born_l = born_base + l;
    };

    const size_t slot_base = (size_t)wave * n_slots;
    const size_t queue_base = (size_t)wave * Q.cap;
    WaveCtx ctx;
    ctx.q_head = 0;
    ctx.q_count = 0;
    ctx.n_dead = n_slots - (uint32_t)slots_per_wave;
    ctx.pool_empty = false;
    ctx.first_rows = (1u << rows) - 1u;
    ctx.first_base = wave * (uint32_t)slots_per_wave;
    ctx.wave = wave;

    bool active = false;
    Walk w;
    w.o = v3(0, 0, 0);
    w.d = v3(0, 0, 1);
    w.inv = v3(0, 0, 0);
    w.pack();
    w.thr = 0.0f;
    w.dest = 0;
    w.best_t = 0.0f;
    w.best_ref = PT_REF_NONE;
    w.set_t_max(FLT_MAX);
    w.cur = PT_REF_NONE;
    w.sp = 0;
    w.occluded = false;
    typename Tracer<STACK_LDS, IN_LDS, true>::Rec rec;
    rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
    float4 win_o = make_float4(0, 0, 0, 0), win_d = make_float4(0, 0, 0, __uint_as_float(PT_DEST_NULL)); // the lane's ray of the ring's window
    uint32_t n_nodes = 0, n_leaves = 0, n_rays = 0, n_shadow = 0, n_samples = 0, n_vertices = 0;
    uint32_t w_steps = 0, w_passes = 0; // wave-level diagnostics (same value in every lane)
#ifdef PT_PATH_TIMING
    unsigned long long t_shade = 0, t_burst = 0, t_inner = 0;
    const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
#endif

    // Two nested loops.  The inner one is the hot path -- retire, hand out queued rays, a burst of traversal steps -- and contains no
    // shading code, so its registers are allocated for it alone; it is left when a shading pass is called for (queue empty, enough
    // slots ready) or when the wavefront has nothing left to do.  The outer one runs the shading pass.
    bool want_pass = false;
    for(;;) {
        if(want_pass) {
            want_pass = false;
            w_passes++;
#ifdef PT_PATH_TIMING
            const unsigned long long t_pass = __builtin_amdgcn_s_memtime();
#endif
            // The pass reads its arguments from *A now (an opaque zero offset keeps the compiler from reading them once, above the
            // traversal loop, and carrying them through it).
            size_t pass_offset = 0;
            asm volatile("" : "+s"(pass_offset));
            const PtPathArgs *P = (const PtPathArgs *)(args_c4)((const char __attribute__((address_space(4))) *)A4 + pass_offset);
            uint32_t *const walk_save = P->walk_save;
            const size_t save_stride = P->save_stride;
            const uint32_t lane_s = lane_afresh(); // (the lane number of the pass)

            // No vector register of the traversal lives across a shading pass (which needs them all): the walks in progress are parked in
            // this lane's column of the save area and read back afterwards.  (The work counters are wavefront totals: scalars, which stay.)
            {
                uint32_t *sv = walk_save + (size_t)wave * 64 + lane_s;
                const size_t st = save_stride;
                sv[0 * st] = __float_as_uint(w.o.x);
                sv[1 * st] = __float_as_uint(w.o.y);
                sv[2 * st] = __float_as_uint(w.o.z);
                sv[3 * st] = __float_as_uint(w.d.x);
                sv[4 * st] = __float_as_uint(w.d.y);
                sv[5 * st] = __float_as_uint(w.d.z);
                sv[6 * st] = __float_as_uint(w.thr);
                sv[7 * st] = w.dest;
                sv[8 * st] = __float_as_uint(w.best_t);
                sv[9 * st] = w.best_ref;
                sv[10 * st] = __float_as_uint(w.t_max);
                sv[11 * st] = w.cur;
                sv[12 * st] = w.sp | (w.occluded ? 0x80000000u : 0u);
            }
            // A pass costs a chain of memory round trips per ROW it visits, however few of the row's slots take part.  Once streams end
            // for good (adaptive sampling stops pixels early; the last streams of any job) the ready slots thin out in every row alike, so
            // when they fit fewer chunks of 64 than they occupy rows, the pass runs over a LIST of them instead (slot numbers in LDS, in
            // slot order): lane i of chunk k shades the (64 k + i)-th ready slot.  Its state accesses are gathers then, which is why a
            // well-filled pass keeps the rows.  (The first round of streams is dealt by row: no list before every row has had its turn.)
            uint32_t n_listed = 0;
            bool compact = false;
            if(PT_COST_LDS_BYTES >= 1024 && !cost_on && P->compact_passes != 0 && rows > 1 && rows <= 4 && ctx.first_rows == 0u) {
                uint32_t rows_used = 0;
                for(uint32_t r = 0; r < (uint32_t)rows; r++) {
                    const typename SW::T word = word_l[r * 64 + lane_s];
                    const bool is_ready = !(SW::flags(word) & PT_F_DONE) && SW::pending(word) == 0;
                    const unsigned long long m = __ballot(is_ready);
                    if(is_ready) {
                        list_l[n_listed + (uint32_t)__popcll(m & ((1ULL << lane_s) - 1ULL))] = (unsigned char)(r * 64 + lane_s);
                    }
                    n_listed += (uint32_t)__popcll(m);
                    rows_used += m != 0ULL ? 1u : 0u;
                }
                compact = (n_listed + 63u) / 64u < rows_used;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // (the list is read by other lanes of this wavefront)
            }
            const uint32_t n_chunks = compact ? (n_listed + 63u) / 64u : (uint32_t)rows;
            // The host's stop request, once per pass: a system-scope load from fine-grained host memory (every lane reads the same word,
            // one request), made a scalar for the whole pass.  The streams see it at their next sample boundary (shade_row).
            uint32_t stop_word = 0;
            if(P->T.cancel != nullptr) {
                stop_word = __hip_atomic_load(P->T.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            const bool stop = __builtin_amdgcn_readfirstlane(stop_word) != 0u;
            // shadow rays are counted where they are queued (every queued ray is walked before the wavefront ends): all the pass queues but
            // the extension rays, which shade_row takes off
            n_shadow -= ctx.q_count;
#pragma unroll 1
            for(uint32_t k = 0; k < n_chunks; k++) {
                // (in a compacted pass `row` is not used: the first round is over)
                uint32_t ls = k * 64u + lane_s;
                if(compact) {
                    ls = ls < n_listed ? (uint32_t)list_l[ls] : PT_NO_SLOT;
                }
                shade_row<WIDE>(P->sc, P->cam, P->opt, P->S, P->T, P->Q, ctx, k, ls, lane_s, (uint32_t)slot_base, queue_base, word_l, hit_l, P->image, P->counters, tb, stop, n_samples, n_vertices, n_shadow);
            }
            n_shadow += ctx.q_count;
            // the rays just written are read back by other lanes of this wavefront
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_s_waitcnt(0);
            {
                // (the save area's address is read again: addresses kept from the stores above would live across the pass, 17 pairs of
                // registers that the pass has no room for)
                asm volatile("" : "+s"(pass_offset));
                const PtPathArgs *R = (const PtPathArgs *)(args_c4)((const char __attribute__((address_space(4))) *)A4 + pass_offset);
                const uint32_t *sv = R->walk_save + (size_t)wave * 64 + lane_afresh();
                const size_t st = R->save_stride;
                w.o = v3(__uint_as_float(sv[0 * st]), __uint_as_float(sv[1 * st]), __uint_as_float(sv[2 * st]));
                w.d = v3(__uint_as_float(sv[3 * st]), __uint_as_float(sv[4 * st]), __uint_as_float(sv[5 * st]));
                w.inv = slab_inverse(w.d);
                w.pack();
                w.thr = __uint_as_float(sv[6 * st]);
                w.dest = sv[7 * st];
                w.best_t = __uint_as_float(sv[8 * st]);
                w.best_ref = sv[9 * st];
                w.set_t_max(__uint_as_float(sv[10 * st]));
                w.cur = sv[11 * st];
                const uint32_t packed = sv[12 * st];
                w.sp = packed & 0x7fffffffu;
                w.occluded = (packed >> 31) != 0;
            }
#ifdef PT_PATH_TIMING
            t_shade += __builtin_amdgcn_s_memtime() - t_pass;
#endif
            // the ring has new rays: its first 64 go to the lanes' window registers (which did not live across the pass)
            win_o = make_float4(0, 0, 0, 0);
            win_d = make_float4(0, 0, 0, __uint_as_float(PT_DEST_NULL));
            const uint32_t lane_w = lane_afresh();
            if(lane_w < ctx.q_count) {
                uint32_t i = ctx.q_head + lane_w;
                i = i >= Q.cap ? i - Q.cap : i;
                win_o = to_f4(ring_o[queue_base + i]);
                win_d = to_f4(ring_d[queue_base + i]);
            }
            // the record registers do not live across a shading pass: walks in progress fetch theirs again
            rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
                    if(active && w.cur < PT_REF_POPPING) { // (a walk that is over or about to pop stands on no record)
                tr.fetch(w.cur, rec);
            }
        }

        {
            size_t bind_offset = 0;
            asm volatile("" : "+s"(bind_offset));
            bind_lane((const PtPathArgs *)(args_c4)((const char __attribute__((address_space(4))) *)A4 + bind_offset), lane_afresh());
        }
        // (One way round the loop and one way out of it -- `leave` -- instead of a break for the pass, one for the end and a continue for a
        // wavefront without walks: with several exits the compiler gave the walk and the record registers a home per exit and moved all of them
        // from one to the next on every trip.)
        bool finished = false;
        bool leave = false;
#ifdef PT_PATH_TIMING
        const unsigned long long t_i0 = __builtin_amdgcn_s_memtime();
#endif
        do {
            // ---- 1. retire finished walks: the result goes to the slot's words in LDS -----------------------------------------------------
            if(active && w.cur == PT_REF_NONE) {
                const uint32_t ls = w.dest & PT_DEST_SLOT_MASK;
                if(w.dest & PT_DEST_SHADOW) {
                    const uint32_t j = (w.dest >> PT_DEST_J_SHIFT) & SW::j_mask;
                    // one ray less pending; an unoccluded light sample sets its visibility bit
                    __hip_atomic_fetch_add(&word_l[ls], (typename SW::T)(w.occluded ? 0u : (1u << j)) - SW::one_ray(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                else {
                    const u2v h = {__float_as_uint(w.best_ref == PT_REF_NONE ? -1.0f : w.best_t), w.best_ref};
                    hit_l[ls] = h;
                    __hip_atomic_fetch_add(&word_l[ls], (typename SW::T)0 - SW::one_ray(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                if(cost_on) {
                    // what the stream cost: the steps this wavefront made while the ray was walking (a stream's rays follow one another,
                    // so their sum is the length of its chain in steps)
                    __hip_atomic_fetch_add(&slot_cost[slot_base + ls], w_steps - *born_l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                active = false;
            }

            // ---- 2. idle lanes: hand out queued rays; with the queue empty, see whether enough slots are ready for a shading pass --------
            const unsigned long long idle_mask = __ballot(!active) & lane_cap;
            const uint32_t n_idle = (uint32_t)__popcll(idle_mask);
            if(n_idle >= (uint32_t)refill_idle) {
                if(ctx.q_count <= (uint32_t)pass_q_low && ctx.n_dead < n_slots) {
                    // slots whose rays have all come back (or that wait for a stream)
                    uint32_t n_ready = 0;
                    for(uint32_t r = 0; r < (uint32_t)rows; r++) {
                        const typename SW::T word = word_l[r * 64 + lane];
                        n_ready += (uint32_t)__popcll(__ballot(!(SW::flags(word) & PT_F_DONE) && SW::pending(word) == 0));
                    }
                    // enough of them for a pass: `min_ready`, or a share of the slots that are still alive -- a wavefront that is down to its
                    // last few streams must not make each of them wait for all the others (their samples are sequential: the launch lasts as
                    // long as its slowest stream)
                    const uint32_t live_share = (n_slots - ctx.n_dead) >> ready_shift;
                    const uint32_t need = live_share < (uint32_t)min_ready ? (live_share > 1u ? live_share : 1u) : (uint32_t)min_ready;
                    // (with rays left in the ring -- pass_q_low > 0 -- the pass is an early one: it tops the ring up before the lanes run dry, and
                    // is only worth its fixed price when `early_ready` slots take part)
                    if(ctx.q_count == 0 ? (n_ready >= need || n_idle == (uint32_t)__popcll(lane_cap)) : n_ready >= (uint32_t)early_ready) {
                        want_pass = true;
                        leave = true;
                    }
                }
                if(!leave && ctx.q_count > 0) {
                    // The ring's next 64 rays are already in registers, one per lane (requested when the ring's head last moved:
                    // reading them here would stall the whole wavefront, walks in progress included, for a memory round trip); an
                    // idle lane takes the ray of the lane whose number is its rank among the idle ones.
                    const uint32_t take = ctx.q_count < n_idle ? ctx.q_count : n_idle;
                    const uint32_t rank = (uint32_t)__popcll(idle_mask & ((1ULL << lane) - 1ULL));
                    const int src = (int)(rank & 63u);
                    // (ds_bpermute, which is what __shfl does for 0 <= src < 64, without the lane number __shfl computes: the compiler
                    // hoisted that out of every loop and kept it in scratch)
                    auto from = [src](float v) { return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v))); };
                    const float4 ro = make_float4(from(win_o.x), from(win_o.y), from(win_o.z), from(win_o.w));
                    const float4 rd = make_float4(from(win_d.x), from(win_d.y), from(win_d.z), from(win_d.w));
                    // The lanes that take a ray, as ONE condition and ONE branch, and the request of the root's record in a branch of its own
                    // behind it.  Nested, each level of branches kept the walk and the record registers of the lanes it skips in a copy: every
                    // refill moved all of them to other registers and back (which also made it wait for the records in flight).
                    const bool take_it = !active & (rank < take) & (__float_as_uint(rd.w) != PT_DEST_NULL);
                    n_rays += (uint32_t)__popcll(__ballot(take_it)); // (rays walked, for the whole wavefront: the branch's own mask)
                    uint32_t first = PT_REF_NONE;
                    if(take_it) {
                        tr.begin(w, root, ro, rd);
                        if(cost_on) {
                            *born_l = w_steps;
                        }
                        active = true;
                        first = w.cur;
                    }
                    asm volatile("" : "+v"(first)); // (opaque: the compiler must not fold the second branch back into the first)
                    if(first != PT_REF_NONE) {
                        tr.fetch(first, rec);
                    }
                    ctx.q_head += take;
                    ctx.q_head = ctx.q_head >= Q.cap ? ctx.q_head - Q.cap : ctx.q_head;
                    ctx.q_count -= take;
                    if(lane < ctx.q_count) {
                        uint32_t i = ctx.q_head + lane;
                        i = i >= Q.cap ? i - Q.cap : i;
                        win_o = to_f4(ring_o[queue_base + i]);
                        win_d = to_f4(ring_d[queue_base + i]);
                    }
                }
            }
            const bool walking = __ballot(active) != 0ULL;
            if(!leave && !walking && ctx.q_count == 0 && ctx.n_dead >= n_slots) {
                finished = true; // every slot is dead, nothing queued, nothing walking
                leave = true;
            }

            // ---- 3. a burst of traversal steps ---------------------------------------------------------------------------------------------
            // Lanes that stand on a leaf wait (their order of visits is unchanged) until `leaf_min` of them can share the leaf code, or no
            // lane has an inner node left; the leaf test then rides along with the other lanes' node step (one memory round trip for both).
#ifdef PT_PATH_TIMING
            const unsigned long long t_b0 = __builtin_amdgcn_s_memtime();
#endif
            // (a lane without a walk in progress has cur == PT_REF_NONE: retire leaves it there, and nothing else changes it)
            // A burst that runs out of walks ends through the loop's own test -- one way out of the loop, a step shorter by its second exit's
            // flag.  The kernels with the wide slot word keep the break: in the other form their shading pass spills two registers more
            // (tests/test_kernel_resources.py; the census of tools/loop_census.py holds both forms at or below what they were).
            if(WIDE) {
#pragma unroll 1
                for(int burst = (!leave && walking) ? 0 : burst_steps; burst < burst_steps; burst++) {
                    w_steps++;
                    if(!tr.step(w, rec, leaf_min, n_nodes, n_leaves)) {
                        w_steps--;
                        break;
                    }
                }
            }
            else {
#pragma unroll 1
                for(int burst = (!leave && walking) ? 0 : burst_steps; burst < burst_steps; burst++) {
                    w_steps++;
                    if(!tr.step(w, rec, leaf_min, n_nodes, n_leaves)) {
                        w_steps--;
                        burst = burst_steps;
                    }
                }
            }
#ifdef PT_PATH_TIMING
            t_burst += __builtin_amdgcn_s_memtime() - t_b0;
#endif
        } while(!leave);
#ifdef PT_PATH_TIMING
        t_inner += __builtin_amdgcn_s_memtime() - t_i0;
#endif
        if(finished) {
            break;
        }
    }

    // Work counters: every wave owns one 64-byte slot (plain stores; atomics on a shared line from every wave serialise at the memory side)
    // (all of them are counted for the whole wavefront)
    if(lane == 0) {
        unsigned long long *slot = A->wave_counters + 8 * (size_t)wave;
        slot[0] += n_nodes;
        slot[1] += n_leaves;
        slot[2] += n_rays;
        slot[3] += n_shadow;
        slot[4] += w_steps;
        slot[5] += w_passes;
        slot[6] += n_samples;
        slot[7] += n_vertices;
#ifdef PT_PATH_TIMING
        // diagnostic build: shader-clock cycles of this wavefront in shading passes, in traversal bursts, in all, and in the inner loop (bursts
        // included: what it spends outside them is retire, pass trigger, hand-out and window reload)
        slot[6] = (unsigned long long)n_samples | ((t_inner >> 10) << 32);
        slot[5] = (unsigned long long)w_passes | ((t_shade >> 10) << 32);
        slot[4] = (unsigned long long)w_steps | ((t_burst >> 10) << 32);
        slot[3] = (unsigned long long)n_shadow | (((__builtin_amdgcn_s_memtime() - t_begin) >> 10) << 32);
        // ... and, of the bursts, in Tracer::slow_step (kilo-cycles), with its invocations, the lanes it served and the trips of its pop loop
        slot[0] = (unsigned long long)n_nodes | ((tr.slow_cycles >> 10) << 32);
        slot[1] = (unsigned long long)n_leaves | ((unsigned long long)tr.slow_calls << 32);
        slot[2] = (unsigned long long)n_rays | ((unsigned long long)tr.slow_served << 32);
        slot[7] = (unsigned long long)n_vertices | ((unsigned long long)tr.slow_trips << 32);
#endif
    }
}

template<bool WIDE, bool IN_LDS, int STACK_LDS>
void launch_path(hipStream_t stream, const PtPathConfig &cfg, const PtPathArgs *d_args) {
    hipLaunchKernelGGL((pt_path_kernel<WIDE, IN_LDS, STACK_LDS>), dim3(cfg.grid), dim3(256), cfg.lds_bytes, stream, d_args);
}

template<bool WIDE, bool IN_LDS, int STACK_LDS>
void occupancy(size_t lds_bytes, int *out) {
    int blocks = 0;
    const hipError_t err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, pt_path_kernel<WIDE, IN_LDS, STACK_LDS>, 256, lds_bytes);
    *out = (err != hipSuccess || blocks < 1) ? 1 : blocks;
}

} // namespace

// the instantiations of the path kernel: slot word (compact | wide) x records (HBM | LDS) x stack window (8 entries; 4 for scenes in LDS that need the room)
#define PT_DISPATCH_PATH(fn, cfg, ...)                                              \
    do {                                                                            \
        if((cfg).in_lds && (cfg).stack_lds == PT_PATH_STACK_LDS_SMALL) {            \
            if((cfg).wide) {                                                        \
                fn<true, true, PT_PATH_STACK_LDS_SMALL>(__VA_ARGS__);               \
            }                                                                       \
            else {                                                                  \
                fn<false, true, PT_PATH_STACK_LDS_SMALL>(__VA_ARGS__);              \
            }                                                                       \
        }                                                                           \
        else if((cfg).in_lds) {                                                     \
            if((cfg).wide) {                                                        \
                fn<true, true, PT_PATH_STACK_LDS>(__VA_ARGS__);                     \
            }                                                                       \
            else {                                                                  \
                fn<false, true, PT_PATH_STACK_LDS>(__VA_ARGS__);                    \
            }                                                                       \
        }                                                                           \
        else {                                                                      \
            if((cfg).wide) {                                                        \
                fn<true, false, PT_PATH_STACK_LDS>(__VA_ARGS__);                    \
            }                                                                       \
            else {                                                                  \
                fn<false, false, PT_PATH_STACK_LDS>(__VA_ARGS__);                   \
            }                                                                       \
        }                                                                           \
    } while(0)

void pt_launch_path(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, const PtDevOptions &options, PtSlots slots, PtStreams streams,
                    PtLocalQueue queue, const PtPathConfig &cfg, float4 *image, PtDevCounters *counters, PtPathArgs *host_args, PtPathArgs *d_args) {
    PtPathArgs &a = *host_args;
    a.sc = scene;
    a.cam = camera;
    a.opt = options;
    a.S = slots;
    a.T = streams;
    a.Q = queue;
    a.rows = cfg.rows;
    a.slots_per_wave = cfg.slots_per_wave;
    a.refill_idle = cfg.refill_idle;
    a.min_ready = cfg.min_ready;
    a.burst_steps = cfg.burst_steps;
    a.leaf_min = cfg.leaf_min;
    a.ready_shift = cfg.ready_shift;
    a.pass_q_low = cfg.pass_q_low;
    a.early_ready = cfg.early_ready;
    a.compact_passes = cfg.compact_passes;
    a.debug_lanes = cfg.debug_lanes;
    a.spill = cfg.spill;
    a.spill_depth = cfg.spill_depth;
    a.save_stride = (uint32_t)cfg.grid * 256u;
    a.walk_save = cfg.walk_save;
    a.image = image;
    a.counters = counters;
    a.wave_counters = cfg.wave_counters;
    (void)hipMemcpyAsync(d_args, host_args, sizeof(PtPathArgs), hipMemcpyHostToDevice, stream);
    PT_DISPATCH_PATH(launch_path, cfg, stream, cfg, d_args);
}

size_t pt_path_lds_bytes(int wide, int rows, int stack_lds, uint32_t n_lds_pairs, uint32_t n_lds_leaf_records) {
    const size_t scene = ((size_t)n_lds_pairs + n_lds_leaf_records) * 64;
    return (size_t)stack_lds * 256 * sizeof(uint2) + (size_t)4 * rows * 64 * (sizeof(uint2) + (wide ? sizeof(unsigned long long) : sizeof(uint32_t))) + PT_LDS_TABLE_BYTES + PT_COST_LDS_BYTES + scene;
}

int pt_path_blocks_per_cu(const PtPathConfig &cfg) {
    int blocks = 1;
    PT_DISPATCH_PATH(occupancy, cfg, cfg.lds_bytes, &blocks);
    return blocks;
}

int pt_path_stack_lds(int in_lds, size_t lds_bytes_with_default_window) {
    // (four workgroups of the path kernel share the 160 KB of a CU when each stays within 40 KB)
    return (in_lds && lds_bytes_with_default_window > 40960) ? PT_PATH_STACK_LDS_SMALL : PT_PATH_STACK_LDS;
}
