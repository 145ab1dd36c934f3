// pt_frames.h -- the resumable frame of the C ABI (include/pt_hip.h), shared by pt_frames.cpp (create, render, progressive passes, queries)
// and pt_frame_maps.cpp (preview, noise and variance maps).  Internal, as pt_host.h.
//
// A frame is a pt_render_tiles_ctl job that keeps what a stop leaves: per replica, the status of every stream after a launch, the park
// records of the streams a stop dropped with samples taken, the work list of the next launch (pt_frame.hip builds it from the status:
// parked streams first, then the untouched ones) and the count of unfinished pixels per tile.  The work list and the park records come in
// pairs that swap on every launch: a launch reads one and writes the other.
#ifndef PT_FRAMES_H
#define PT_FRAMES_H

#include "pt_host.h"

struct pt_frame {
    // One map of the frame (pt_frame_maps.cpp), per replica: the entries its gather kernel makes of the replica's work list, in one or two
    // arrays on the replica's own device, and the fixed-size summary the kernel may write next to them; on replica 0 also the other
    // replicas' entries on their way in
    struct Entries {
        size_t size[2];         // bytes of an entry in each array (0: the map has no second array); must be the sizes of the types the
                                // map's two callables cast own[] and stage[] to -- nothing else checks them
        size_t summary_words;   // (0: no summary)
        pth::DevBuf<uint8_t> own[2], stage[2];
        pth::DevBuf<uint32_t> summary;
    };
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
        pth::DevBuf<int4> d_tiles;
        pth::DevBuf<uint32_t> d_offset, d_left, d_status, d_blocks, d_park_count;
        pth::DevBuf<uint2> d_todo[2];
        pth::DevBuf<PtParkRecord> d_park[2];
        pth::DevBuf<unsigned long long> d_result;
        pth::DevBuf<PtViewCamera> d_view_cams; // a view frame's tables
        pth::DevBuf<uint64_t> d_view_seeds;
        // the maps' entries: preview (colour; pixel and samples), noise (pixel and error bits; the summary), variance (variance; pixel)
        Entries preview{{sizeof(pth::F4), sizeof(int2)}, 0}, noise{{sizeof(uint2), 0}, PT_NOISE_SUMMARY_WORDS}, variance{{sizeof(pth::F4), sizeof(int32_t)}, 0};
        bool previewed = false; // device buffers of the maps exist (on replica 0's device whether or not the replica has rendered)
        // on replica 0, the maps themselves: the frame's view and sample counts, its error map, its variance map; which pixels a tile
        // covers; the frame's first-hit features
        pth::DevBuf<pth::F4> pv_view, pv_features, vr_map;
        pth::DevBuf<int32_t> pv_samples;
        pth::DevBuf<float> nz_map;
        pth::DevBuf<uint8_t> cover;
        bool cover_ready = false, pv_features_ready = false;
    };
    pt_camera_params camera{};
    pt_options options{};
    std::vector<pt_tile> tiles;
    uint64_t base_seed = 0;
    // a frame over a view batch (pt_frame_create_views, V > 1): the image is the V frames stacked, `views` the frame's own copy of the
    // cameras and seeds (every replica keeps them in device tables of its own: the scene's are any other batch's to overwrite between two
    // slices) and `cameras` what the preview's feature pass takes.  A plain frame has n_views = 1 and no tables.
    int32_t n_views = 1;
    pth::ViewSet views;
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

    // what every call but pt_frame_get_info makes of a failed frame (the mutex held)
    int check() const { return status != PT_OK ? pth::fail(status, error) : PT_OK; }
};

namespace pth {
// A progressive frame's list split again by the sample count `yield_at` and the noise target as they are now, with nothing launched and
// no record moved (pt_frames.cpp): before a pass of a frame with a noise target, and behind the list a loaded checkpoint rebuilds
int frame_resort(pt_frame &f, pt_frame::Replica &r, int32_t yield_at);
} // namespace pth

#endif
