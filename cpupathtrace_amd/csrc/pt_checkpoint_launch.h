// pt_checkpoint_launch.h -- the launches of pt_checkpoint.hip, for pt_checkpoint.cpp.  Each returns 0, or 1 when a launch failed.
#ifndef PT_CHECKPOINT_LAUNCH_H
#define PT_CHECKPOINT_LAUNCH_H

#include <hip/hip_runtime.h>

#include "pt_types.h"

// words of block_sums a replica of n streams needs (pack uses 2 per workgroup of 1024 streams, unpack 3), and of `partials`
size_t pt_checkpoint_block_words(uint32_t n_streams);
size_t pt_checkpoint_partial_words(uint32_t n_streams);

// PACK, on `stream`: from the replica's work list todo[0 .. n_todo) and the records it names in park[0 .. park_cap), the map byte of each
// of its n_streams streams (slot: n_streams words of scratch), and -- unless out_records is null: the sizes only -- the finished pixels
// gathered from `image` (`width` wide) and the trimmed records as 16-byte units, both in the replica's stream order.
// max_pixels / max_units: the room behind out_pixels and out_records.  tile_finished /
// tile_units [n_tiles]: the finished streams and record units before each tile's first stream; totals [PT_CKPT_TOTALS].
int pt_launch_checkpoint_pack(hipStream_t stream, const uint2 *todo, uint32_t n_todo, const PtParkRecord *park, uint32_t park_cap, uint32_t n_streams, uint32_t *slot,
                              uint32_t *block_sums, const float4 *image, const int4 *tiles, const uint32_t *tile_offset, uint32_t n_tiles, int32_t width, uint8_t *map,
                              float4 *out_pixels, uint4 *out_records, unsigned long long max_pixels, unsigned long long max_units, unsigned long long *tile_finished, unsigned long long *tile_units, unsigned long long *totals);

// UNPACK, on `stream`: from the replica's n_streams map bytes and its trimmed records, the work list (todo [n_streams]) and the full park
// records (park: one per stream with a record), and per workgroup of 1024 streams the list's summary (partials, PT_CKPT_PARTIALS each).
int pt_launch_checkpoint_unpack(hipStream_t stream, const uint8_t *map, uint32_t n_streams, uint32_t *block_sums, const uint4 *trimmed, uint2 *todo, PtParkRecord *park,
                                unsigned long long *partials);

#endif
