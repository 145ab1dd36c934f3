// pt_checkpoint_format.cpp -- layout, writer and parser of a frame checkpoint's blob (pt_checkpoint_format.h; the format is stated in
// include/pt_checkpoint.h), and pt_checkpoint_inspect.  No HIP: this unit also builds as an ordinary host program.
#include "pt_checkpoint_format.h"

#include <cmath>
#include <cstring>

namespace ptc {

namespace {

constexpr uint64_t kMaxStreams = 0x0fffffffull; // what a frame takes (check_tiles)
constexpr uint64_t kFullRecord = PT_CHECKPOINT_RECORD_BYTES + 8ull * PT_CHECKPOINT_CANDIDATE_BYTES;
constexpr uint32_t kSizeEstimator = 128, kSizeCandidate = 48, kMaxCandidates = 8;
static_assert(sizeof(pt_checkpoint_header) == 352, "the header has no implicit padding");
static_assert(sizeof(pt_checkpoint_fingerprint) == 72, "the fingerprint has no implicit padding");
static_assert(sizeof(pt_tile) == 16 && sizeof(pt_options) == 20 && sizeof(pt_camera_params) == 68, "the job's structs as the format states them");

int bad(const std::string &field, const std::string &why) {
    return pth::fail(PT_ERR_INVALID, "checkpoint: " + field + ": " + why);
}

// a + b and a * b into *out; false on overflow
bool add(uint64_t a, uint64_t b, uint64_t *out) { return !__builtin_add_overflow(a, b, out); }
bool mul(uint64_t a, uint64_t b, uint64_t *out) { return !__builtin_mul_overflow(a, b, out); }
bool align16(uint64_t a, uint64_t *out) {
    uint64_t up;
    if(!add(a, 15, &up)) {
        return false;
    }
    *out = up & ~15ull;
    return true;
}

bool all_zero(const uint8_t *p, size_t n) {
    for(size_t i = 0; i < n; i++) {
        if(p[i] != 0) {
            return false;
        }
    }
    return true;
}

} // namespace

uint64_t checksum(const void *bytes, size_t n) {
    const uint8_t *p = static_cast<const uint8_t *>(bytes);
    const size_t words = n / 8;
    auto step = [](uint64_t h, uint64_t v) {
        h ^= v;
        h *= 0x100000001b3ull;
        return h ^ (h >> 32);
    };
    uint64_t h[8];
    for(uint64_t l = 0; l < 8; l++) {
        h[l] = 0xcbf29ce484222325ull + l;
    }
    size_t i = 0;
    for(; i + 8 <= words; i += 8) {
        uint64_t w[8];
        std::memcpy(w, p + 8 * i, 64); // (little-endian hosts only, as the rest of the library)
        for(int l = 0; l < 8; l++) {
            h[l] = step(h[l], w[l]);
        }
    }
    for(int l = 0; i < words; i++, l++) {
        uint64_t w;
        std::memcpy(&w, p + 8 * i, 8);
        h[l] = step(h[l], w);
    }
    for(int l = 1; l < 8; l++) {
        h[0] = step(h[0], h[l]);
    }
    return h[0];
}

int layout(const pt_checkpoint_header &h, Layout *out) {
    Layout l;
    uint64_t at = sizeof(pt_checkpoint_header), end = 0;
    l.tables = static_cast<size_t>(at);
    l.seeds = l.tables;
    if(h.n_views > 1) {
        uint64_t cams, seeds, seeds_at;
        if(!mul(static_cast<uint64_t>(h.n_views), sizeof(pt_camera_params), &cams) || !add(at, cams, &end) || !align16(end, &seeds_at) ||
           !mul(static_cast<uint64_t>(h.n_views), 8, &seeds) || !add(seeds_at, seeds, &end) || h.bytes_tables != end - at) {
            return bad("bytes_tables", "not what n_views cameras and seeds take");
        }
        l.seeds = static_cast<size_t>(seeds_at);
    }
    else if(h.bytes_tables != 0) {
        return bad("bytes_tables", "a frame of one view has no tables");
    }
    const uint64_t sizes[4] = {h.bytes_tiles, h.bytes_map, h.bytes_pixels, h.bytes_records};
    size_t *starts[4] = {&l.tiles, &l.map, &l.pixels, &l.records};
    static const char *const names[4] = {"bytes_tiles", "bytes_map", "bytes_pixels", "bytes_records"};
    uint64_t prev = h.bytes_tables;
    for(int i = 0; i < 4; i++) {
        if(!add(at, prev, &end) || !align16(end, &at)) {
            return bad(names[i], "the sections before it overflow");
        }
        *starts[i] = static_cast<size_t>(at);
        prev = sizes[i];
    }
    uint64_t total;
    if(!add(at, prev, &end) || !align16(end, &at) || !add(at, 8, &total)) {
        return bad("bytes_records", "the blob's size overflows");
    }
    l.trailer = static_cast<size_t>(at);
    l.total = static_cast<size_t>(total);
    *out = l;
    return PT_OK;
}

int fill_sizes(pt_checkpoint_header *h, uint64_t record_bytes) {
    std::memcpy(h->magic, PT_CHECKPOINT_MAGIC, 8);
    h->version = PT_CHECKPOINT_VERSION;
    h->header_bytes = sizeof(pt_checkpoint_header);
    h->size_estimator = kSizeEstimator;
    h->size_candidate = kSizeCandidate;
    h->max_candidates = kMaxCandidates;
    h->size_camera = sizeof(pt_camera_params);
    h->size_options = sizeof(pt_options);
    h->bytes_tables = 0;
    if(h->n_views > 1) {
        h->bytes_tables = ((static_cast<uint64_t>(h->n_views) * sizeof(pt_camera_params) + 15) & ~15ull) + static_cast<uint64_t>(h->n_views) * 8;
    }
    if(!mul(h->n_tiles, sizeof(pt_tile), &h->bytes_tiles) || !mul(h->streams_finished, 16, &h->bytes_pixels)) {
        return bad("n_tiles", "too many");
    }
    h->bytes_map = h->n_streams;
    h->bytes_records = record_bytes;
    h->total_bytes = 0;
    Layout l;
    const int rc = layout(*h, &l);
    if(rc != PT_OK) {
        return rc;
    }
    h->total_bytes = l.total;
    return PT_OK;
}

int start(void *blob, size_t capacity, const pt_checkpoint_header &h, const pt_camera_params *cams, const uint64_t *seeds, const pt_tile *tiles, Layout *out) {
    Layout l;
    const int rc = layout(h, &l);
    if(rc != PT_OK) {
        return rc;
    }
    if(blob == nullptr || capacity < l.total || h.total_bytes != l.total) {
        return bad("capacity", "the blob takes " + std::to_string(l.total) + " bytes");
    }
    uint8_t *b = static_cast<uint8_t *>(blob);
    std::memcpy(b, &h, sizeof(h));
    if(h.n_views > 1) {
        const size_t n = static_cast<size_t>(h.n_views);
        std::memcpy(b + l.tables, cams, n * sizeof(pt_camera_params));
        std::memset(b + l.tables + n * sizeof(pt_camera_params), 0, l.seeds - (l.tables + n * sizeof(pt_camera_params)));
        std::memcpy(b + l.seeds, seeds, n * 8);
    }
    if(h.n_tiles != 0) {
        std::memcpy(b + l.tiles, tiles, static_cast<size_t>(h.bytes_tiles));
    }
    // the padding behind every section
    const size_t ends[5] = {l.tables + static_cast<size_t>(h.bytes_tables), l.tiles + static_cast<size_t>(h.bytes_tiles), l.map + static_cast<size_t>(h.bytes_map),
                            l.pixels + static_cast<size_t>(h.bytes_pixels), l.records + static_cast<size_t>(h.bytes_records)};
    const size_t nexts[5] = {l.tiles, l.map, l.pixels, l.records, l.trailer};
    for(int i = 0; i < 5; i++) {
        std::memset(b + ends[i], 0, nexts[i] - ends[i]);
    }
    *out = l;
    return PT_OK;
}

void seal(void *blob, const Layout &l) {
    const uint64_t sum = checksum(blob, l.trailer);
    std::memcpy(static_cast<uint8_t *>(blob) + l.trailer, &sum, 8);
}

int write(void *blob, size_t capacity, pt_checkpoint_header h, const pt_camera_params *cams, const uint64_t *seeds, const pt_tile *tiles, const uint8_t *map,
          const void *pixels, const void *records, uint64_t record_bytes, size_t *written) {
    h.streams_finished = h.streams_untouched = h.streams_with_record = 0;
    for(uint64_t i = 0; i < h.n_streams; i++) {
        const unsigned c = map_class(map[i]);
        h.streams_finished += c == PT_CHECKPOINT_FINISHED ? 1 : 0;
        h.streams_untouched += c == PT_CHECKPOINT_UNTOUCHED ? 1 : 0;
        h.streams_with_record += c == PT_CHECKPOINT_RECORD ? 1 : 0;
    }
    int rc = fill_sizes(&h, record_bytes);
    if(rc != PT_OK) {
        return rc;
    }
    if(written != nullptr) {
        *written = static_cast<size_t>(h.total_bytes);
    }
    Layout l;
    rc = start(blob, capacity, h, cams, seeds, tiles, &l);
    if(rc != PT_OK) {
        return rc;
    }
    uint8_t *b = static_cast<uint8_t *>(blob);
    if(h.bytes_map != 0) {
        std::memcpy(b + l.map, map, static_cast<size_t>(h.bytes_map));
    }
    if(h.bytes_pixels != 0) {
        std::memcpy(b + l.pixels, pixels, static_cast<size_t>(h.bytes_pixels));
    }
    if(h.bytes_records != 0) {
        std::memcpy(b + l.records, records, static_cast<size_t>(h.bytes_records));
    }
    seal(blob, l);
    return PT_OK;
}

int parse(const void *blob, size_t bytes, Parsed *out, bool per_tile) {
    if(blob == nullptr) {
        return pth::fail(PT_ERR_INVALID, "checkpoint: null blob");
    }
    if(bytes < sizeof(pt_checkpoint_header) + 8) {
        return bad("total_bytes", "shorter than a header and a trailer");
    }
    const uint8_t *b = static_cast<const uint8_t *>(blob);
    Parsed local;
    Parsed &p = out != nullptr ? *out : local;
    pt_checkpoint_header &h = p.h;
    std::memcpy(&h, b, sizeof(h));
    if(std::memcmp(h.magic, PT_CHECKPOINT_MAGIC, 8) != 0) {
        return bad("magic", "not a frame checkpoint");
    }
    if(h.version != PT_CHECKPOINT_VERSION) {
        return bad("version", std::to_string(h.version) + " (this build reads " + std::to_string(PT_CHECKPOINT_VERSION) + ")");
    }
    if(h.header_bytes != sizeof(pt_checkpoint_header)) {
        return bad("header_bytes", std::to_string(h.header_bytes));
    }
    if(h.size_estimator != kSizeEstimator) {
        return bad("size_estimator", std::to_string(h.size_estimator));
    }
    if(h.size_candidate != kSizeCandidate) {
        return bad("size_candidate", std::to_string(h.size_candidate));
    }
    if(h.max_candidates != kMaxCandidates) {
        return bad("max_candidates", std::to_string(h.max_candidates));
    }
    if(h.size_camera != sizeof(pt_camera_params)) {
        return bad("size_camera", std::to_string(h.size_camera));
    }
    if(h.size_options != sizeof(pt_options)) {
        return bad("size_options", std::to_string(h.size_options));
    }
    if(h.total_bytes != bytes) {
        return bad("total_bytes", std::to_string(h.total_bytes) + " in a blob of " + std::to_string(bytes));
    }
    // the job
    if(h.n_views < 1) {
        return bad("n_views", std::to_string(h.n_views));
    }
    if(h.options.image_width <= 0 || h.options.image_height <= 0) {
        return bad("options", "the image size must be positive");
    }
    const uint64_t rows = static_cast<uint64_t>(h.n_views) * static_cast<uint64_t>(h.options.image_height);
    if(rows > 0x7fffffffull) {
        return bad("n_views", "more than 2^31 - 1 rows");
    }
    if(h.n_streams > kMaxStreams) {
        return bad("n_streams", "more than 0x0fffffff");
    }
    if(h.n_tiles > h.n_streams) {
        return bad("n_tiles", "more tiles than streams");
    }
    uint64_t sum;
    if(!add(h.streams_finished, h.streams_untouched, &sum) || !add(sum, h.streams_with_record, &sum) || sum != h.n_streams) {
        return bad("streams_finished", "streams_finished + streams_untouched + streams_with_record is not n_streams");
    }
    if(h.bytes_tiles != h.n_tiles * sizeof(pt_tile)) {
        return bad("bytes_tiles", "not 16 bytes for each of n_tiles");
    }
    if(h.bytes_map != h.n_streams) {
        return bad("bytes_map", "not one byte for each of n_streams");
    }
    if(h.bytes_pixels != h.streams_finished * 16) {
        return bad("bytes_pixels", "not 16 bytes for each of streams_finished");
    }
    if(h.bytes_records < h.streams_with_record * PT_CHECKPOINT_RECORD_BYTES || h.bytes_records > h.streams_with_record * kFullRecord) {
        return bad("bytes_records", "outside what streams_with_record records can take");
    }
    int rc = layout(h, &p.at);
    if(rc != PT_OK) {
        return rc;
    }
    const Layout &l = p.at;
    if(l.total != bytes) {
        return bad("total_bytes", "the sections (bytes_tables, bytes_tiles, bytes_map, bytes_pixels, bytes_records) take " + std::to_string(l.total) + " bytes");
    }
    // the mode
    const int32_t progressive[4] = {h.quantum, h.max_passes_per_call, h.passes_completed, h.target};
    static const char *const progressive_names[4] = {"quantum", "max_passes_per_call", "passes_completed", "target"};
    for(int i = 0; i < 4; i++) {
        if(progressive[i] < 0) {
            return bad(progressive_names[i], "negative");
        }
    }
    if(h.pass_in_progress != 0 && h.pass_in_progress != 1) {
        return bad("pass_in_progress", std::to_string(h.pass_in_progress));
    }
    if(!std::isfinite(h.noise_target) || h.noise_target < 0.0f) {
        return bad("noise_target", "must be finite and not negative");
    }
    if(!std::isfinite(h.noise_floor) || h.noise_floor < 0.0f) {
        return bad("noise_floor", "must be finite and not negative");
    }
    if(!(h.noise_fraction > 0.0f && h.noise_fraction <= 1.0f)) {
        return bad("noise_fraction", "must be in (0, 1]");
    }
    if(h.follow_features != 0 && h.follow_features != 1) {
        return bad("follow_features", std::to_string(h.follow_features));
    }
    if(h.feature_params.max_bounces < 0 || h.feature_params.max_bounces > 32 || h.feature_params.flags != 0) {
        return bad("feature_params", "outside what pt_frame_set_feature_params takes");
    }
    if(h.launches < 0) {
        return bad("launches", std::to_string(h.launches));
    }
    p.cams = b + l.tables;
    p.seeds = b + l.seeds;
    p.tiles = b + l.tiles;
    p.map = b + l.map;
    p.pixels = b + l.pixels;
    p.records = b + l.records;
    // the tiles: inside the image, and their pixels are the map's streams
    const size_t n_tiles = static_cast<size_t>(h.n_tiles);
    if(per_tile) {
        p.tile_stream.assign(n_tiles + 1, 0);
        p.tile_finished.assign(n_tiles + 1, 0);
        p.tile_records.assign(n_tiles + 1, 0);
        p.tile_record_bytes.assign(n_tiles + 1, 0);
    }
    uint64_t streams = 0;
    for(size_t k = 0; k < n_tiles; k++) {
        pt_tile t;
        std::memcpy(&t, p.tiles + k * sizeof(pt_tile), sizeof(t));
        if(t.w <= 0 || t.h <= 0 || t.x < 0 || t.y < 0 || static_cast<int64_t>(t.x) + t.w > h.options.image_width || static_cast<uint64_t>(static_cast<int64_t>(t.y) + t.h) > rows) {
            return bad("tiles", "tile " + std::to_string(k) + " is empty or outside the image");
        }
        streams += static_cast<uint64_t>(t.w) * static_cast<uint64_t>(t.h); // (at most 2^62 per tile: the test below ends the loop long before a wrap)
        if(streams > h.n_streams) {
            return bad("tiles", "more pixels than n_streams");
        }
    }
    if(streams != h.n_streams) {
        return bad("tiles", "their pixels are not n_streams");
    }
    // the map, tile by tile
    uint64_t finished = 0, untouched = 0, with_record = 0, record_bytes = 0, s = 0;
    p.with_candidates = 0;
    for(size_t k = 0; k < n_tiles; k++) {
        pt_tile t;
        std::memcpy(&t, p.tiles + k * sizeof(pt_tile), sizeof(t));
        if(per_tile) {
            p.tile_stream[k] = s;
            p.tile_finished[k] = finished;
            p.tile_records[k] = with_record;
            p.tile_record_bytes[k] = record_bytes;
        }
        const uint64_t end = s + static_cast<uint64_t>(t.w) * static_cast<uint64_t>(t.h);
        for(; s < end; s++) {
            const uint8_t m = p.map[s];
            const unsigned c = map_class(m), cand = map_candidates(m);
            if(c > PT_CHECKPOINT_RECORD || (m & 0xc0u) != 0 || cand > kMaxCandidates || (cand != 0 && c != PT_CHECKPOINT_RECORD)) {
                return bad("map", "byte " + std::to_string(s) + " is " + std::to_string(m));
            }
            if(c == PT_CHECKPOINT_FINISHED) {
                finished++;
            }
            else if(c == PT_CHECKPOINT_UNTOUCHED) {
                untouched++;
            }
            else {
                with_record++;
                record_bytes += PT_CHECKPOINT_RECORD_BYTES + cand * PT_CHECKPOINT_CANDIDATE_BYTES;
                p.with_candidates += cand != 0 ? 1 : 0;
            }
        }
    }
    if(per_tile) {
        p.tile_stream[n_tiles] = s;
        p.tile_finished[n_tiles] = finished;
        p.tile_records[n_tiles] = with_record;
        p.tile_record_bytes[n_tiles] = record_bytes;
    }
    if(finished != h.streams_finished || untouched != h.streams_untouched || with_record != h.streams_with_record) {
        return bad("map", "its classes are not the header's counts");
    }
    if(record_bytes != h.bytes_records) {
        return bad("bytes_records", "the map implies " + std::to_string(record_bytes));
    }
    // the records name the candidates the map says they have
    uint64_t at = 0;
    for(uint64_t i = 0; i < h.n_streams && with_record != 0; i++) {
        if(map_class(p.map[i]) != PT_CHECKPOINT_RECORD) {
            continue;
        }
        const unsigned cand = map_candidates(p.map[i]);
        int32_t n_candidates;
        std::memcpy(&n_candidates, p.records + at + 16 + 116, 4); // (PtEstimator::n_candidates)
        if(n_candidates != static_cast<int32_t>(cand)) {
            return bad("records", "the record of stream " + std::to_string(i) + " has " + std::to_string(n_candidates) + " candidates, its map byte " + std::to_string(cand));
        }
        at += PT_CHECKPOINT_RECORD_BYTES + cand * PT_CHECKPOINT_CANDIDATE_BYTES;
    }
    // the padding
    const size_t cams_end = h.n_views > 1 ? l.tables + static_cast<size_t>(h.n_views) * sizeof(pt_camera_params) : l.tables;
    const size_t ends[6] = {cams_end, l.tables + static_cast<size_t>(h.bytes_tables), l.tiles + static_cast<size_t>(h.bytes_tiles), l.map + static_cast<size_t>(h.bytes_map),
                            l.pixels + static_cast<size_t>(h.bytes_pixels), l.records + static_cast<size_t>(h.bytes_records)};
    const size_t nexts[6] = {h.n_views > 1 ? l.seeds : l.tables, l.tiles, l.map, l.pixels, l.records, l.trailer};
    for(int i = 0; i < 6; i++) {
        if(!all_zero(b + ends[i], nexts[i] - ends[i])) {
            return bad("padding", "not 0 behind section " + std::to_string(i));
        }
    }
    uint64_t stored;
    std::memcpy(&stored, b + l.trailer, 8);
    if(stored != checksum(b, l.trailer)) {
        return bad("checksum", "the blob is damaged");
    }
    return PT_OK;
}

} // namespace ptc

extern "C" int pt_checkpoint_inspect(const void *blob, size_t bytes, pt_checkpoint_info *out) {
    if(blob == nullptr || out == nullptr) {
        return pth::fail(PT_ERR_INVALID, "checkpoint: null argument");
    }
    ptc::Parsed p;
    const int rc = ptc::parse(blob, bytes, &p, false);
    if(rc != PT_OK) {
        return rc;
    }
    const pt_checkpoint_header &h = p.h;
    std::memset(out, 0, sizeof(*out));
    out->total_bytes = h.total_bytes;
    out->n_tiles = h.n_tiles;
    out->n_streams = h.n_streams;
    out->streams_finished = h.streams_finished;
    out->streams_untouched = h.streams_untouched;
    out->streams_with_record = h.streams_with_record;
    out->streams_with_candidates = p.with_candidates;
    out->bytes_header = h.header_bytes;
    out->bytes_tables = h.bytes_tables;
    out->bytes_tiles = h.bytes_tiles;
    out->bytes_map = h.bytes_map;
    out->bytes_pixels = h.bytes_pixels;
    out->bytes_records = h.bytes_records;
    out->samples_lost = h.samples_lost;
    out->fingerprint = h.fingerprint;
    out->options = h.options;
    out->version = h.version;
    out->n_views = h.n_views;
    out->quantum = h.quantum;
    out->max_passes_per_call = h.max_passes_per_call;
    out->passes_completed = h.passes_completed;
    out->target = h.target;
    out->pass_in_progress = h.pass_in_progress;
    out->noise_target = h.noise_target;
    out->noise_floor = h.noise_floor;
    out->noise_fraction = h.noise_fraction;
    out->follow_features = h.follow_features;
    out->launches = h.launches;
    return PT_OK;
}
