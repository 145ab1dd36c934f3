// pt_checkpoint_format.h -- the blob of a frame checkpoint (include/pt_checkpoint.h has the format): its layout, writer
// and parser.  Host code that knows nothing of HIP and nothing of pt_host.h beyond the error codes and the message of a failure, so that
// it is compiled, tested and run under sanitizers where there is no device (tests/cpp/checkpoint_fuzz.cpp, tests/checkpoint_probe.py).
#ifndef PT_CHECKPOINT_FORMAT_H
#define PT_CHECKPOINT_FORMAT_H

#include "../../include/pt_hip.h"

#include <string>
#include <vector>

namespace pth {
// the calling thread's message (pt_last_error); defined in pt_api.cpp, and by every stand-alone program that links this unit
int fail(int code, const std::string &msg);
} // namespace pth

namespace ptc {

// Where the sections of a blob are, from the counts of its header
struct Layout {
    size_t tables = 0, seeds = 0, tiles = 0, map = 0, pixels = 0, records = 0, trailer = 0, total = 0;
};
// PT_OK, or PT_ERR_INVALID naming the count that does not fit a size_t or contradicts another
int layout(const pt_checkpoint_header &h, Layout *out);

// The sizes and the magic of this build into h, and the byte counts of its sections from its stream counts, n_tiles, n_views and
// `record_bytes`; then total_bytes.  PT_ERR_INVALID when a count overflows.
int fill_sizes(pt_checkpoint_header *h, uint64_t record_bytes);

// Writes header, tables and tiles of a blob of h.total_bytes and zeroes the padding behind every section (the map's, the pixels' and
// the records' too); the caller then fills map, pixels and records at out's offsets and calls seal.  cams / seeds: n_views of each for
// a view frame, else unused.
int start(void *blob, size_t capacity, const pt_checkpoint_header &h, const pt_camera_params *cams, const uint64_t *seeds, const pt_tile *tiles, Layout *out);
void seal(void *blob, const Layout &l);
uint64_t checksum(const void *bytes, size_t n); // n a multiple of 8

// The whole writer over plain arrays: map[n_streams], pixels[16 * finished] and the trimmed records as the format lays them out.
// `h` carries the job, the mode, the counters and the fingerprint; its sizes and counts are filled here.
int write(void *blob, size_t capacity, pt_checkpoint_header h, const pt_camera_params *cams, const uint64_t *seeds, const pt_tile *tiles, const uint8_t *map,
          const void *pixels, const void *records, uint64_t record_bytes, size_t *written);

// Bounded views of a validated blob.  Every pointer points into [blob, blob + bytes).
struct Parsed {
    pt_checkpoint_header h; // a copy (the blob need not be aligned)
    Layout at;
    const uint8_t *cams = nullptr, *seeds = nullptr, *tiles = nullptr, *map = nullptr, *pixels = nullptr, *records = nullptr;
    uint64_t with_candidates = 0;
    // per tile of the frame's list, and one past the last: its first stream, and the finished streams, the records and the record bytes
    // before it
    std::vector<uint64_t> tile_stream, tile_finished, tile_records, tile_record_bytes;
};
// Validates everything include/pt_checkpoint.h lists, in that order, and fills `out` (may be null: validation only).  `per_tile`: fill
// the per-tile vectors as well.
int parse(const void *blob, size_t bytes, Parsed *out, bool per_tile);

inline unsigned map_class(uint8_t b) { return b & 3u; }
inline unsigned map_candidates(uint8_t b) { return (b >> 2) & 15u; }

} // namespace ptc

#endif
