// pt_checkpoint.hip -- the two device steps of a frame checkpoint (pt_frame_checkpoint_save / _load, pt_checkpoint.cpp): pack and unpack.
// The kernels are pt_checkpoint_kernels.h; this file launches them.
#include "pt_checkpoint_kernels.h"
#include "pt_checkpoint_launch.h"

size_t pt_checkpoint_block_words(uint32_t n_streams) {
    return 3 * (((size_t)n_streams + kCkPerBlock - 1) / kCkPerBlock);
}

size_t pt_checkpoint_partial_words(uint32_t n_streams) {
    return PT_CKPT_PARTIALS * (((size_t)n_streams + kCkPerBlock - 1) / kCkPerBlock);
}

int pt_launch_checkpoint_pack(hipStream_t stream, const uint2 *todo, uint32_t n_todo, const PtParkRecord *park, uint32_t park_cap, uint32_t n_streams, uint32_t *slot,
                              uint32_t *block_sums, const float4 *image, const int4 *tiles, const uint32_t *tile_offset, uint32_t n_tiles, int32_t width, uint8_t *map,
                              float4 *out_pixels, uint4 *out_records, unsigned long long max_pixels, unsigned long long max_units, unsigned long long *tile_finished, unsigned long long *tile_units, unsigned long long *totals) {
    if(hipMemsetAsync(totals, 0, PT_CKPT_TOTALS * sizeof(unsigned long long), stream) != hipSuccess ||
       (n_streams != 0 && hipMemsetAsync(slot, 0, (size_t)n_streams * sizeof(uint32_t), stream) != hipSuccess)) {
        return 1;
    }
    if(n_streams == 0) {
        return 0;
    }
    if(n_todo != 0) {
        pt_checkpoint_mark_kernel<<<(n_todo + kCkThreads - 1) / kCkThreads, kCkThreads, 0, stream>>>(todo, n_todo, n_streams, slot);
    }
    const uint32_t n_blocks = (n_streams + kCkPerBlock - 1) / kCkPerBlock;
    pt_checkpoint_classify_kernel<<<n_blocks, kCkThreads, 0, stream>>>(slot, n_streams, park, park_cap, map, block_sums, totals);
    pt_checkpoint_gather_kernel<<<n_blocks, kCkThreads, 0, stream>>>(slot, n_streams, map, block_sums, park, image, tiles, tile_offset, n_tiles, width, out_pixels,
                                                                    out_records, max_pixels, max_units, tile_finished, tile_units, totals);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int pt_launch_checkpoint_unpack(hipStream_t stream, const uint8_t *map, uint32_t n_streams, uint32_t *block_sums, const uint4 *trimmed, uint2 *todo, PtParkRecord *park,
                                unsigned long long *partials) {
    if(n_streams == 0) {
        return 0;
    }
    const uint32_t n_blocks = (n_streams + kCkPerBlock - 1) / kCkPerBlock;
    pt_checkpoint_count_kernel<<<n_blocks, kCkThreads, 0, stream>>>(map, n_streams, block_sums);
    pt_checkpoint_expand_kernel<<<n_blocks, kCkThreads, 0, stream>>>(map, n_streams, block_sums, n_blocks, trimmed, todo, park, partials);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
