// pt_checkpoint.cpp -- checkpoints of a resumable frame (include/pt_checkpoint.h): pt_frame_checkpoint_size, _save and
// _load over pt_frames.h.  The blob's format is pt_checkpoint_format.cpp's (no HIP there); the device steps are pt_checkpoint.hip's.
//
// SAVE packs every replica on its own device and stream under the scene's render_mutex: the replica's work list and park records give
// the map bytes, the finished pixels and the trimmed records in the replica's stream order, with the offsets of every tile.  A tile
// belongs to one replica and its streams are contiguous in the frame's order, so the blob is the tiles' segments copied into that order.
// LOAD deals the blob's tiles as pt_frame_create does, hands every replica its tiles' segments, and unpacks them into a work list (records
// first, then the untouched streams, both in stream order) and full park records; a progressive frame's list is then split by the
// frame's target with the work-list kernel (frame_resort), which also finds what a noise target holds.
#include "pt_frames.h"

#include "pt_checkpoint_format.h"
#include "pt_checkpoint_kernels.h" // (the PT_CKPT_* words; its kernels are pt_checkpoint.hip's)
#include "pt_checkpoint_launch.h"

using namespace pth;

namespace {

static_assert(sizeof(PtEstimator) == 128 && sizeof(PtCandidate) == 48 && PT_MAX_CANDIDATES == 8 && sizeof(PtParkRecord) == 16 + 128 + 8 * 48,
              "the sizes the format states (pt_checkpoint_format.cpp)");

pt_checkpoint_fingerprint fingerprint_of(const pt_scene *s) {
    pt_checkpoint_fingerprint fp{};
    fp.triangles = s->dev.n_tris;
    fp.spheres = s->dev.n_spheres;
    fp.materials = s->dev.n_materials;
    fp.point_lights = s->dev.n_lights;
    fp.emitters = s->dev.n_emis;
    fp.tree_nodes = s->n_nodes;
    for(int k = 0; k < 3; k++) {
        fp.root_box[k] = bits(s->dev.root_lo[k]);
        fp.root_box[3 + k] = bits(s->dev.root_hi[k]);
    }
    return fp;
}

int fingerprint_check(const pt_checkpoint_fingerprint &want, const pt_scene *s, int scene) {
    const pt_checkpoint_fingerprint got = fingerprint_of(s);
    const uint64_t a[6] = {want.triangles, want.spheres, want.materials, want.point_lights, want.emitters, want.tree_nodes};
    const uint64_t b[6] = {got.triangles, got.spheres, got.materials, got.point_lights, got.emitters, got.tree_nodes};
    static const char *const names[6] = {"triangles", "spheres", "materials", "point_lights", "emitters", "tree_nodes"};
    for(int k = 0; k < 6; k++) {
        if(a[k] != b[k]) {
            return fail(PT_ERR_INVALID, std::string("checkpoint: fingerprint.") + names[k] + ": the blob's scene has " + std::to_string(a[k]) + ", scene " +
                                            std::to_string(scene) + " has " + std::to_string(b[k]));
        }
    }
    if(std::memcmp(want.root_box, got.root_box, sizeof(want.root_box)) != 0) {
        return fail(PT_ERR_INVALID, "checkpoint: fingerprint.root_box: scene " + std::to_string(scene) + " has another root box");
    }
    return PT_OK;
}

// What pack left of one replica: on the host the small tables, on the replica's device the three sections in its stream order
struct Packed {
    std::vector<unsigned long long> tile_finished, tile_units; // per tile of the replica, and one past the last
    uint64_t finished = 0, units = 0;
    bool on_device = false; // (a replica that never launched, or has no tiles: every stream untouched, nothing on the device)
    DevBuf<uint8_t> map;
    DevBuf<F4> pixels;
    DevBuf<uint4> records;
};

// Pack one replica (the frame's lock held).  sizes_only: no pixel and no record moves, `image` is not read.
int pack_replica(const pt_frame &f, pt_frame::Replica &r, const float *image, bool sizes_only, Packed *out) {
    const size_t n_tiles = r.tiles.size();
    out->tile_finished.assign(n_tiles + 1, 0);
    out->tile_units.assign(n_tiles + 1, 0);
    if(!r.ready || r.n_streams == 0) {
        return PT_OK;
    }
    pt_scene *s = r.s;
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    const uint32_t n = r.n_streams;
    const uint64_t n_finished = n - r.n_todo;
    if(!sizes_only && n_finished != 0) {
        const size_t pixels = static_cast<size_t>(f.options.image_width) * static_cast<size_t>(f.rows());
        PT_HIP(s->image.ensure(pixels));
        // (to the device only: the caller's image is read)
        PT_TRY(copy_tile_rects(s, r.tiles, r.index, nullptr, const_cast<float *>(image), static_cast<size_t>(f.options.image_width), true));
    }
    DevBuf<uint32_t> slot, sums;
    DevBuf<unsigned long long> tile_finished, tile_units, totals;
    PT_HIP(slot.ensure(n));
    PT_HIP(sums.ensure(pt_checkpoint_block_words(n)));
    PT_HIP(tile_finished.ensure(n_tiles));
    PT_HIP(tile_units.ensure(n_tiles));
    PT_HIP(totals.ensure(PT_CKPT_TOTALS));
    PT_HIP(out->map.ensure(n));
    if(!sizes_only) {
        PT_HIP(out->pixels.ensure(n_finished));
        PT_HIP(out->records.ensure(static_cast<size_t>(r.n_parked) * PT_CKPT_FULL_UNITS));
    }
    const uint32_t park_cap = static_cast<uint32_t>(std::min<size_t>(r.d_park[r.pcur].count, 0x0fffffffu));
    PT_LAUNCH(pt_launch_checkpoint_pack(s->stream, r.d_todo[r.cur].ptr, r.n_todo, r.d_park[r.pcur].ptr, r.d_park[r.pcur].ptr != nullptr ? park_cap : 0u, n, slot.ptr, sums.ptr,
                                        reinterpret_cast<const float4 *>(s->image.ptr), r.d_tiles.ptr, r.d_offset.ptr, static_cast<uint32_t>(n_tiles),
                                        f.options.image_width, out->map.ptr, reinterpret_cast<float4 *>(out->pixels.ptr), sizes_only ? nullptr : out->records.ptr,
                                        sizes_only ? 0ull : n_finished, sizes_only ? 0ull : static_cast<uint64_t>(r.n_parked) * PT_CKPT_FULL_UNITS, tile_finished.ptr, tile_units.ptr, totals.ptr),
              "checkpoint: pack kernels failed to launch");
    unsigned long long t[PT_CKPT_TOTALS];
    PT_HIP(hipMemcpyAsync(t, totals.ptr, sizeof(t), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipMemcpyAsync(out->tile_finished.data(), tile_finished.ptr, n_tiles * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipMemcpyAsync(out->tile_units.data(), tile_units.ptr, n_tiles * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    if(t[PT_CKPT_TOTAL_BAD] != 0 || t[PT_CKPT_TOTAL_FINISHED] != n_finished || t[PT_CKPT_TOTAL_UNITS] > static_cast<uint64_t>(r.n_parked) * PT_CKPT_FULL_UNITS) {
        return fail(PT_ERR_HIP, "checkpoint: the work list of a replica names " + std::to_string(t[PT_CKPT_TOTAL_FINISHED]) + " finished streams of " +
                                    std::to_string(n_finished) + " and " + std::to_string(t[PT_CKPT_TOTAL_UNITS]) + " record units");
    }
    out->finished = t[PT_CKPT_TOTAL_FINISHED];
    out->units = t[PT_CKPT_TOTAL_UNITS];
    out->tile_finished[n_tiles] = out->finished;
    out->tile_units[n_tiles] = out->units;
    out->on_device = true;
    return PT_OK;
}

// The header of the frame as it stands, without the counts pack gives
pt_checkpoint_header header_of(const pt_frame &f) {
    pt_checkpoint_header h{};
    h.n_views = f.n_views;
    h.n_tiles = f.tiles.size();
    h.n_streams = f.streams_total;
    h.base_seed = f.base_seed;
    h.options = f.options;
    h.camera = f.camera;
    h.quantum = f.quantum;
    h.max_passes_per_call = f.max_passes_per_call;
    h.passes_completed = f.passes_completed;
    h.target = f.target;
    h.pass_in_progress = f.pass_in_progress ? 1 : 0;
    h.noise_target = f.noise_target;
    h.noise_floor = f.noise_floor;
    h.noise_fraction = f.noise_fraction;
    h.follow_features = f.follow_features ? 1 : 0;
    h.feature_params = f.feature_params;
    h.launches = f.launches;
    h.samples_lost = f.samples_lost;
    h.fingerprint = fingerprint_of(f.reps[0]->s);
    return h;
}

// Frees what pack left on the replicas' devices, each on its own
void release(const pt_frame &f, std::vector<Packed> &packed) {
    for(size_t i = 0; i < packed.size(); i++) {
        if(packed[i].on_device) {
            (void)hipSetDevice(f.reps[i]->s->device);
            packed[i].map.release();
            packed[i].pixels.release();
            packed[i].records.release();
        }
    }
}

// pt_frame_checkpoint_size (blob null) and _save, the frame's lock held
int save_locked(pt_frame &f, const float *image, void *blob, size_t capacity, size_t *written) {
    const bool sizes_only = blob == nullptr;
    std::vector<Packed> packed(f.reps.size());
    struct Release {
        const pt_frame &f;
        std::vector<Packed> &p;
        ~Release() { release(f, p); }
    } guard{f, packed};
    pt_checkpoint_header h = header_of(f);
    uint64_t units = 0;
    for(size_t i = 0; i < f.reps.size(); i++) {
        pt_frame::Replica &r = *f.reps[i];
        PT_TRY(pack_replica(f, r, image, sizes_only, &packed[i]));
        h.streams_finished += packed[i].finished;
        h.streams_with_record += packed[i].on_device ? r.n_parked : 0;
        units += packed[i].units;
    }
    h.streams_untouched = h.n_streams - h.streams_finished - h.streams_with_record;
    PT_TRY(ptc::fill_sizes(&h, units * 16));
    if(written != nullptr) {
        *written = static_cast<size_t>(h.total_bytes);
    }
    if(sizes_only) {
        return PT_OK;
    }
    if(capacity < h.total_bytes) {
        return fail(PT_ERR_INVALID, "checkpoint: capacity: the blob takes " + std::to_string(h.total_bytes) + " bytes");
    }
    std::vector<pt_camera_params> cams;
    if(f.n_views > 1) {
        cams = f.cameras;
    }
    ptc::Layout at;
    PT_TRY(ptc::start(blob, capacity, h, cams.data(), f.views.seeds.data(), f.tiles.data(), &at));
    uint8_t *const b = static_cast<uint8_t *>(blob);
    // where every tile's segments go: the frame's order
    std::vector<uint64_t> first(f.tiles.size() + 1, 0), fin_before(f.tiles.size() + 1, 0), units_before(f.tiles.size() + 1, 0);
    std::vector<int> owner(f.tiles.size(), 0);
    std::vector<size_t> local(f.tiles.size(), 0);
    for(size_t i = 0; i < f.reps.size(); i++) {
        for(size_t k = 0; k < f.reps[i]->index.size(); k++) {
            owner[f.reps[i]->index[k]] = static_cast<int>(i);
            local[f.reps[i]->index[k]] = k;
        }
    }
    for(size_t k = 0; k < f.tiles.size(); k++) {
        const Packed &p = packed[static_cast<size_t>(owner[k])];
        const size_t l = local[k];
        first[k + 1] = first[k] + static_cast<uint64_t>(f.tiles[k].w) * static_cast<uint64_t>(f.tiles[k].h);
        fin_before[k + 1] = fin_before[k] + (p.tile_finished[l + 1] - p.tile_finished[l]);
        units_before[k + 1] = units_before[k] + (p.tile_units[l + 1] - p.tile_units[l]);
    }
    for(size_t i = 0; i < f.reps.size(); i++) {
        pt_frame::Replica &r = *f.reps[i];
        Packed &p = packed[i];
        if(!p.on_device) {
            for(size_t k = 0; k < r.index.size(); k++) {
                std::memset(b + at.map + first[r.index[k]], static_cast<int>(PT_CHECKPOINT_UNTOUCHED), static_cast<size_t>(first[r.index[k] + 1] - first[r.index[k]]));
            }
            continue;
        }
        pt_scene *s = r.s;
        std::lock_guard<std::mutex> lock(s->render_mutex);
        PT_HIP(hipSetDevice(s->device));
        // runs of tiles that follow each other in the replica's order and in the frame's: one copy per section each
        for(size_t k = 0; k < r.index.size();) {
            size_t e = k + 1;
            while(e < r.index.size() && r.index[e] == r.index[e - 1] + 1) {
                e++;
            }
            const size_t g = r.index[k];
            const uint64_t s0 = first[g], s1 = first[r.index[e - 1] + 1];
            uint64_t local_first = 0;
            for(size_t j = 0; j < k; j++) {
                local_first += static_cast<uint64_t>(r.tiles[j].w) * static_cast<uint64_t>(r.tiles[j].h);
            }
            PT_HIP(hipMemcpyAsync(b + at.map + s0, p.map.ptr + local_first, static_cast<size_t>(s1 - s0), hipMemcpyDeviceToHost, s->stream));
            const uint64_t nf = p.tile_finished[e] - p.tile_finished[k], nu = p.tile_units[e] - p.tile_units[k];
            if(nf != 0) {
                PT_HIP(hipMemcpyAsync(b + at.pixels + 16 * fin_before[g], p.pixels.ptr + p.tile_finished[k], static_cast<size_t>(16 * nf), hipMemcpyDeviceToHost, s->stream));
            }
            if(nu != 0) {
                PT_HIP(hipMemcpyAsync(b + at.records + 16 * units_before[g], p.records.ptr + p.tile_units[k], static_cast<size_t>(16 * nu), hipMemcpyDeviceToHost, s->stream));
            }
            k = e;
        }
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    ptc::seal(blob, at);
    return PT_OK;
}

// The device tables of a loaded replica (what frame_prepare of pt_frames.cpp makes for a fresh one) and its unpacked list and records
// (its tiles' segments of the blob's map and records go to the device run by run, as a save brings them back)
int unpack_replica(pt_frame &f, pt_frame::Replica &r, const ptc::Parsed &p, const std::vector<uint32_t> &left, uint32_t n_records, uint32_t n_untouched,
                   uint64_t record_bytes) {
    pt_scene *s = r.s;
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    StreamDrain drain{s->stream};
    const uint32_t n = r.n_streams;
    const TileTable table(r.tiles.data(), r.tiles.size());
    if(f.n_views > 1) {
        PT_HIP(r.d_view_cams.upload(f.views.cams));
        PT_HIP(r.d_view_seeds.upload(f.views.seeds));
    }
    PT_HIP(r.d_tiles.upload(table.rects));
    PT_HIP(r.d_offset.upload(table.offsets));
    PT_HIP(r.d_left.upload(left));
    PT_HIP(r.d_todo[0].ensure(n));
    PT_HIP(r.d_todo[1].ensure(n));
    PT_HIP(r.d_status.ensure(n));
    PT_HIP(hipMemset(r.d_status.ptr, 0, static_cast<size_t>(n) * sizeof(uint32_t)));
    PT_HIP(r.d_blocks.ensure(pt_checkpoint_block_words(n))); // (three words per 1024 streams: the work-list kernels' size as well)
    PT_HIP(r.d_park_count.ensure(1));
    PT_HIP(r.d_park[0].ensure(n_records));
    PT_HIP(r.d_result.ensure(PT_COMPACT_WORDS));
    DevBuf<uint8_t> d_map;
    DevBuf<uint4> d_trimmed;
    DevBuf<unsigned long long> d_partials;
    PT_HIP(d_map.ensure(n));
    PT_HIP(d_trimmed.ensure(static_cast<size_t>(record_bytes / 16)));
    uint64_t map_at = 0, records_at = 0;
    for(size_t k = 0; k < r.index.size();) {
        size_t e = k + 1;
        while(e < r.index.size() && r.index[e] == r.index[e - 1] + 1) {
            e++;
        }
        const size_t g0 = r.index[k], g1 = r.index[e - 1] + 1;
        const uint64_t n_map = p.tile_stream[g1] - p.tile_stream[g0], n_rec = p.tile_record_bytes[g1] - p.tile_record_bytes[g0];
        PT_HIP(hipMemcpyAsync(d_map.ptr + map_at, p.map + p.tile_stream[g0], static_cast<size_t>(n_map), hipMemcpyHostToDevice, s->stream));
        if(n_rec != 0) {
            PT_HIP(hipMemcpyAsync(reinterpret_cast<uint8_t *>(d_trimmed.ptr) + records_at, p.records + p.tile_record_bytes[g0], static_cast<size_t>(n_rec), hipMemcpyHostToDevice,
                                  s->stream));
        }
        map_at += n_map;
        records_at += n_rec;
        k = e;
    }
    const size_t n_partials = pt_checkpoint_partial_words(n);
    PT_HIP(d_partials.ensure(n_partials));
    PT_LAUNCH(pt_launch_checkpoint_unpack(s->stream, d_map.ptr, n, r.d_blocks.ptr, d_trimmed.ptr, r.d_todo[0].ptr, r.d_park[0].ptr, d_partials.ptr),
              "checkpoint: unpack kernels failed to launch");
    std::vector<unsigned long long> partials(n_partials);
    PT_HIP(hipMemcpyAsync(partials.data(), d_partials.ptr, n_partials * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    drain.armed = false;
    // the list's summary, as frame_launch reads it from the work-list kernel's result words
    unsigned long long carried = 0, with_candidates = 0, least = 0xffffffffull, most = 0;
    for(size_t b = 0; b < n_partials / PT_CKPT_PARTIALS; b++) {
        const unsigned long long *p = partials.data() + PT_CKPT_PARTIALS * b;
        carried += p[PT_CKPT_CARRIED];
        with_candidates += p[PT_CKPT_WITH_CANDIDATES];
        least = std::min(least, p[PT_CKPT_MIN]);
        most = std::max(most, p[PT_CKPT_MAX]);
    }
    r.cur = 0;
    r.pcur = 0;
    r.n_todo = n_records + n_untouched;
    r.n_parked = n_records;
    r.n_held = 0;
    r.n_at_target = 0;
    r.in_order = r.n_todo == r.n_streams && (r.n_parked == 0 || r.n_parked == r.n_todo);
    r.samples_carried = carried;
    r.with_candidates = with_candidates;
    r.min_samples = r.n_todo != 0 ? static_cast<int32_t>(least) : 0;
    r.max_samples = static_cast<int32_t>(most);
    r.ready = true;
    return PT_OK;
}

int load_impl(pt_scene *const *scenes, int n_scenes, const void *blob, size_t bytes, float *out_image, std::unique_ptr<pt_frame> &f) {
    ptc::Parsed p;
    PT_TRY(ptc::parse(blob, bytes, &p, true));
    const pt_checkpoint_header &h = p.h;
    for(int i = 0; i < n_scenes; i++) {
        PT_TRY(fingerprint_check(h.fingerprint, scenes[i], i));
    }
    PtDevOptions opt;
    PT_TRY(derive_options(&h.options, &opt));
    if(device_count_quiet() < 1) {
        return fail(PT_ERR_NO_DEVICE, "pt_frame_checkpoint_load: no HIP device (a frame renders on the GPU only)");
    }
    const size_t n_tiles = static_cast<size_t>(h.n_tiles);
    f.reset(new pt_frame());
    f->camera = h.camera;
    f->options = h.options;
    f->tiles.resize(n_tiles);
    if(n_tiles != 0) {
        std::memcpy(f->tiles.data(), p.tiles, n_tiles * sizeof(pt_tile));
    }
    f->base_seed = h.base_seed;
    if(h.n_views > 1) {
        const size_t v = static_cast<size_t>(h.n_views);
        std::vector<pt_camera_params> cams(v);
        std::vector<uint64_t> seeds(v);
        std::memcpy(cams.data(), p.cams, v * sizeof(pt_camera_params));
        std::memcpy(seeds.data(), p.seeds, v * 8);
        std::vector<pt_tile> tiles;
        PT_TRY(prepare_views(cams.data(), seeds.data(), h.n_views, &h.options, &tiles, &f->views));
        if(tiles.size() != n_tiles || (n_tiles != 0 && std::memcmp(tiles.data(), f->tiles.data(), n_tiles * sizeof(pt_tile)) != 0)) {
            return fail(PT_ERR_INVALID, "checkpoint: tiles: not the tiles of a frame of " + std::to_string(h.n_views) + " views");
        }
        f->n_views = h.n_views;
        f->cameras = cams;
    }
    f->tile_done.assign(n_tiles, 0);
    f->streams_total = h.n_streams;
    for(int i = 0; i < n_scenes; i++) {
        f->reps.emplace_back(new pt_frame::Replica());
        f->reps.back()->s = scenes[i];
    }
    const std::vector<int> owners = n_tiles > 0 ? tile_owners(f->tiles.data(), n_tiles, n_scenes) : std::vector<int>();
    for(size_t k = 0; k < n_tiles; k++) {
        pt_frame::Replica &r = *f->reps[static_cast<size_t>(owners[k])];
        r.tiles.push_back(f->tiles[k]);
        r.index.push_back(k);
        r.n_streams += static_cast<uint32_t>(f->tiles[k].w) * static_cast<uint32_t>(f->tiles[k].h);
    }
    // the mode and the counters
    f->quantum = h.quantum;
    f->max_passes_per_call = h.max_passes_per_call;
    f->passes_completed = h.passes_completed;
    f->target = h.target;
    f->pass_in_progress = h.pass_in_progress != 0;
    f->noise_target = h.noise_target;
    f->noise_floor = h.noise_floor;
    f->noise_fraction = h.noise_fraction;
    f->follow_features = h.follow_features != 0;
    f->feature_params = h.feature_params;
    f->launches = h.launches;
    f->samples_lost = h.samples_lost;
    // every replica's tiles: their segments of the map and of the records, end to end in the replica's order
    for(auto &rp : f->reps) {
        pt_frame::Replica &r = *rp;
        r.n_todo = r.n_streams;
        if(r.n_streams == 0) {
            continue;
        }
        std::vector<uint32_t> left(r.tiles.size());
        uint64_t n_records = 0, n_finished = 0, record_bytes = 0;
        for(size_t k = 0; k < r.index.size(); k++) {
            const size_t g = r.index[k];
            const uint64_t fin = p.tile_finished[g + 1] - p.tile_finished[g];
            left[k] = static_cast<uint32_t>(p.tile_stream[g + 1] - p.tile_stream[g] - fin);
            f->tile_done[g] = left[k] == 0 ? 1 : 0;
            n_finished += fin;
            n_records += p.tile_records[g + 1] - p.tile_records[g];
            record_bytes += p.tile_record_bytes[g + 1] - p.tile_record_bytes[g];
        }
        PT_TRY(unpack_replica(*f, r, p, left, static_cast<uint32_t>(n_records), static_cast<uint32_t>(r.n_streams - n_finished - n_records), record_bytes));
    }
    f->tiles_done = static_cast<uint64_t>(std::count(f->tile_done.begin(), f->tile_done.end(), 1));
    // a progressive frame's list is split by its target: streams below it, streams at it, streams the noise target holds
    if(f->quantum > 0 && f->target > 0) {
        for(auto &r : f->reps) {
            PT_TRY(frame_resort(*f, *r, f->target));
        }
    }
    // the finished pixels, into the caller's image
    const size_t width = static_cast<size_t>(h.options.image_width);
    uint64_t at = 0;
    for(size_t k = 0; k < n_tiles; k++) {
        const pt_tile &t = f->tiles[k];
        for(uint64_t i = p.tile_stream[k]; i < p.tile_stream[k + 1]; i++) {
            if(ptc::map_class(p.map[i]) != PT_CHECKPOINT_FINISHED) {
                continue;
            }
            const uint64_t local = i - p.tile_stream[k];
            const size_t x = static_cast<size_t>(t.x) + static_cast<size_t>(local % static_cast<uint64_t>(t.w));
            const size_t y = static_cast<size_t>(t.y) + static_cast<size_t>(local / static_cast<uint64_t>(t.w));
            std::memcpy(out_image + 4 * (y * width + x), p.pixels + 16 * at, 16);
            at++;
        }
    }
    return PT_OK;
}

} // namespace

extern "C" {

int pt_frame_checkpoint_size(pt_frame *f, size_t *bytes) {
    if(f == nullptr || bytes == nullptr) {
        return fail(PT_ERR_INVALID, "checkpoint: null argument");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    PT_TRY(f->check());
    return save_locked(*f, nullptr, nullptr, 0, bytes);
}

int pt_frame_checkpoint_save(pt_frame *f, const float *image, void *blob, size_t capacity, size_t *written) {
    if(written != nullptr) {
        *written = 0;
    }
    if(f == nullptr || image == nullptr || blob == nullptr) {
        return fail(PT_ERR_INVALID, "checkpoint: null argument");
    }
    std::lock_guard<std::mutex> lock(f->mutex);
    PT_TRY(f->check());
    return save_locked(*f, image, blob, capacity, written);
}

int pt_frame_checkpoint_load(pt_scene *const *scenes, int n_scenes, const void *blob, size_t bytes, float *out_image, pt_frame **out) {
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
    if(blob == nullptr || out_image == nullptr) {
        return fail(PT_ERR_INVALID, "checkpoint: null argument");
    }
    std::unique_ptr<pt_frame> f;
    const int rc = load_impl(scenes, n_scenes, blob, bytes, out_image, f);
    if(rc != PT_OK) {
        // (no frame and no leak: a replica's buffers go on its own device, once its stream is idle; live_frames was not counted yet)
        if(f != nullptr) {
            const std::string why = last_error();
            for(auto &r : f->reps) {
                std::lock_guard<std::mutex> lock(r->s->render_mutex);
                (void)hipSetDevice(r->s->device);
                (void)hipStreamSynchronize(r->s->stream);
                r.reset();
            }
            f.reset();
            return fail(rc, why);
        }
        return rc;
    }
    for(auto &r : f->reps) {
        r->s->live_frames.fetch_add(1); // (as pt_frame_create)
    }
    *out = f.release();
    return PT_OK;
}

} // extern "C"
