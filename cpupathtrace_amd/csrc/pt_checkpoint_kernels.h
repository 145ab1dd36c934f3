// pt_checkpoint_kernels.h -- the device side of a frame checkpoint (include/pt_checkpoint.h): PACK turns a replica's work
// list, park records and image into the blob's map bytes, finished pixels and trimmed records in the replica's stream order; UNPACK turns
// those back into a work list and full park records.  Included by exactly one translation unit of the library, pt_checkpoint.hip.
//
// What is decided per stream or per 16-byte unit is a PT_D function; the __global__ wrappers add the scans (a workgroup scan in LDS plus
// one pass over the sums of the workgroups before, as the work-list kernels of pt_frame.hip do with block_counts; no atomics, nothing
// depends on the order in which workgroups run).  tests/hip/checkpoint_probe.hip compiles the PT_D functions alone for the host
// (PT_CHECKPOINT_HOST) and runs them under a serial scan of its own.
//
// A record moves as 16-byte units, ONE LANE PER UNIT: unit j of a trimmed record is unit j of the park record (33 units: stream header,
// 8 of the estimator, 3 per candidate), so a wavefront reads runs of 9..33 consecutive units and writes 64 consecutive ones.
#ifndef PT_CHECKPOINT_KERNELS_H
#define PT_CHECKPOINT_KERNELS_H

#include <hip/hip_runtime.h>

#include "pt_types.h"

#ifndef PT_D
#define PT_D __device__ __forceinline__
#endif

#define PT_CKPT_FINISHED 0u
#define PT_CKPT_UNTOUCHED 1u
#define PT_CKPT_RECORD 2u
#define PT_CKPT_HEAD_UNITS 9u   // 16 bytes of cursor and engine, 128 of the estimator
#define PT_CKPT_CAND_UNITS 3u
#define PT_CKPT_FULL_UNITS 33u

// the summary of a replica's unpacked list, per workgroup (the host adds them up)
enum PtCheckpointPartial { PT_CKPT_CARRIED = 0, PT_CKPT_WITH_CANDIDATES, PT_CKPT_MIN, PT_CKPT_MAX, PT_CKPT_PARTIALS };
// what pack's last workgroup leaves: finished streams, record units, list entries that name no record of the buffer (none)
enum PtCheckpointTotal { PT_CKPT_TOTAL_FINISHED = 0, PT_CKPT_TOTAL_UNITS, PT_CKPT_TOTAL_BAD, PT_CKPT_TOTALS };

namespace ptd {

// What a work-list entry says of its stream, in the coding of PtStreams::status: untouched, or 2 + its record
PT_D uint32_t ckpt_slot(uint2 e) {
    return e.y == PT_NO_PARK ? PT_CKPT_UNTOUCHED : PT_CKPT_RECORD + e.y;
}

// The map byte of a stream with slot value `slot` (0: absent from the list, finished).  A record index outside the buffer reads nothing:
// the stream counts as untouched and *bad is set.
PT_D uint8_t ckpt_map_byte(uint32_t slot, const PtParkRecord *park, uint32_t park_cap, uint32_t *bad) {
    if(slot < PT_CKPT_RECORD) {
        return (uint8_t)slot;
    }
    const uint32_t rec = slot - PT_CKPT_RECORD;
    if(rec >= park_cap) {
        *bad = 1u;
        return (uint8_t)PT_CKPT_UNTOUCHED;
    }
    int32_t k = park[rec].est.n_candidates;
    k = k < 0 ? 0 : (k > PT_MAX_CANDIDATES ? PT_MAX_CANDIDATES : k);
    return (uint8_t)(PT_CKPT_RECORD | ((uint32_t)k << 2));
}

// 16-byte units of the trimmed record a map byte stands for
PT_D uint32_t ckpt_units(uint8_t m) {
    return (m & 3u) == PT_CKPT_RECORD ? PT_CKPT_HEAD_UNITS + PT_CKPT_CAND_UNITS * ((uint32_t)(m >> 2) & 15u) : 0u;
}

// Unit j of the trimmed form of *rec (j < 9 + 3 * n_candidates): the park record's unit j, but (cursor, rng, 0) for the header and zeros
// in the pad words
PT_D uint4 ckpt_pack_unit(const PtParkRecord *rec, uint32_t j) {
    uint4 v = reinterpret_cast<const uint4 *>(rec)[j];
    if(j == 0u) {
        v = make_uint4(v.y, v.z, v.w, 0u);
    }
    else if(j == PT_CKPT_HEAD_UNITS - 1u) {
        v.w = 0u; // PtEstimator::pad
    }
    else if(j >= PT_CKPT_HEAD_UNITS && (j - PT_CKPT_HEAD_UNITS) % PT_CKPT_CAND_UNITS == 2u) {
        v = make_uint4(v.x, 0u, 0u, 0u); // PtCandidate::count, pad[3]
    }
    return v;
}

// Unit j (< 33) of the full park record of `stream` whose trimmed form with k candidates starts at `trimmed`: unwritten candidate slots
// are zeros
PT_D uint4 ckpt_unpack_unit(const uint4 *trimmed, uint32_t k, uint32_t stream, uint32_t j) {
    if(j >= PT_CKPT_HEAD_UNITS + PT_CKPT_CAND_UNITS * k) {
        return make_uint4(0u, 0u, 0u, 0u);
    }
    uint4 v = trimmed[j];
    if(j == 0u) {
        v = make_uint4(stream, v.x, v.y, v.z);
    }
    return v;
}

// The tile of stream `stream` of a replica (the last tile whose first stream is not behind it, as stream_pixel of pt_frame.hip) and its
// pixel in an image `width` wide
PT_D uint32_t ckpt_stream_tile(uint32_t stream, const uint32_t *tile_offset, uint32_t n_tiles) {
    uint32_t lo = 0, hi = n_tiles;
    while(hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if(tile_offset[mid] <= stream) {
            lo = mid;
        }
        else {
            hi = mid;
        }
    }
    return lo;
}
PT_D size_t ckpt_stream_pixel(uint32_t stream, uint32_t tile, const int4 *tiles, const uint32_t *tile_offset, int32_t width) {
    const int4 t = tiles[tile];
    const uint32_t k = stream - tile_offset[tile];
    const int32_t x = t.x + (int32_t)(k % (uint32_t)t.z), y = t.y + (int32_t)(k / (uint32_t)t.z);
    return (size_t)y * (size_t)width + (size_t)x;
}

// pixel_sample of a trimmed record (unit 8 of it: remaining_checks, n_candidates, pixel_sample, pad)
PT_D int32_t ckpt_samples(const uint4 *trimmed) {
    return (int32_t)trimmed[PT_CKPT_HEAD_UNITS - 1u].z;
}

} // namespace ptd

#ifndef PT_CHECKPOINT_HOST

namespace {

constexpr uint32_t kCkThreads = 256;
constexpr uint32_t kCkPerThread = 4;
constexpr uint32_t kCkPerBlock = kCkThreads * kCkPerThread;

// Inclusive scan of `mine` over the workgroup's threads in thread order (scan: kCkThreads words of LDS)
__device__ unsigned long long ckpt_block_scan(unsigned long long mine, unsigned long long *scan) {
    scan[threadIdx.x] = mine;
    __syncthreads();
    for(uint32_t d = 1; d < kCkThreads; d <<= 1) {
        const unsigned long long add = threadIdx.x >= d ? scan[threadIdx.x - d] : 0ull;
        __syncthreads();
        scan[threadIdx.x] += add;
        __syncthreads();
    }
    return scan[threadIdx.x];
}

// The sum of `mine` over the workgroup, for every thread (red: kCkThreads words of LDS)
__device__ unsigned long long ckpt_block_sum(unsigned long long mine, unsigned long long *red) {
    __syncthreads();
    red[threadIdx.x] = mine;
    __syncthreads();
    for(uint32_t d = kCkThreads / 2; d > 0; d >>= 1) {
        if(threadIdx.x < d) {
            red[threadIdx.x] += red[threadIdx.x + d];
        }
        __syncthreads();
    }
    const unsigned long long sum = red[0];
    __syncthreads();
    return sum;
}

// ---- pack ---------------------------------------------------------------------------------------------------------------------------------

// One thread per entry of the work list: slot[stream] = what the entry says (slot starts as zeros: a stream no entry names is finished)
__global__ __launch_bounds__(kCkThreads) void pt_checkpoint_mark_kernel(const uint2 *__restrict__ todo, uint32_t n, uint32_t n_streams, uint32_t *__restrict__ slot) {
    const uint32_t i = blockIdx.x * kCkThreads + threadIdx.x;
    if(i < n) {
        const uint2 e = todo[i];
        if(e.x < n_streams) {
            slot[e.x] = ptd::ckpt_slot(e);
        }
    }
}

// Four streams per thread: their map bytes, and per workgroup the finished streams and the record units (block_sums: [2 * workgroups])
__global__ __launch_bounds__(kCkThreads) void pt_checkpoint_classify_kernel(const uint32_t *__restrict__ slot, uint32_t n_streams, const PtParkRecord *__restrict__ park,
                                                                            uint32_t park_cap, uint8_t *__restrict__ map, uint32_t *__restrict__ block_sums,
                                                                            unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long red[kCkThreads];
    unsigned long long mine = 0;
    uint32_t bad = 0;
    for(uint32_t k = 0; k < kCkPerThread; k++) {
        const uint32_t s = blockIdx.x * kCkPerBlock + threadIdx.x * kCkPerThread + k;
        if(s < n_streams) {
            const uint8_t m = ptd::ckpt_map_byte(slot[s], park, park_cap, &bad);
            map[s] = m;
            mine += ((m & 3u) == PT_CKPT_FINISHED ? 1ull : 0ull) + ((unsigned long long)ptd::ckpt_units(m) << 32);
        }
    }
    if(bad != 0) {
        totals[PT_CKPT_TOTAL_BAD] = 1ull; // (every writer writes the same value)
    }
    const unsigned long long sum = ckpt_block_sum(mine, red);
    if(threadIdx.x == 0) {
        block_sums[2 * blockIdx.x] = (uint32_t)sum;
        block_sums[2 * blockIdx.x + 1] = (uint32_t)(sum >> 32);
    }
}

// The same four streams per thread, from their map bytes: the finished pixels and the trimmed records to their places in the replica's
// stream order, and per tile the finished streams and the record units before its first stream.  out_records: null = the sizes only.
// max_pixels / max_units: the room the host made from its own counts; nothing is read or written for a pixel or a unit beyond it (the
// host compares the totals with its counts afterwards and fails the call if they differ).
__global__ __launch_bounds__(kCkThreads) void pt_checkpoint_gather_kernel(const uint32_t *__restrict__ slot, uint32_t n_streams, const uint8_t *__restrict__ map,
                                                                          const uint32_t *__restrict__ block_sums, const PtParkRecord *__restrict__ park,
                                                                          const float4 *__restrict__ image, const int4 *__restrict__ tiles,
                                                                          const uint32_t *__restrict__ tile_offset, uint32_t n_tiles, int32_t width,
                                                                          float4 *__restrict__ out_pixels, uint4 *__restrict__ out_records,
                                                                          unsigned long long max_pixels, unsigned long long max_units,
                                                                          unsigned long long *__restrict__ tile_finished, unsigned long long *__restrict__ tile_units,
                                                                          unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long scan[kCkThreads];
    __shared__ uint32_t start[kCkPerBlock + 1]; // record units of the workgroup before each of its streams
    __shared__ uint32_t source[kCkPerBlock];    // ... and the stream's record
    unsigned long long fin_before = 0, units_before = 0;
    for(uint32_t b = threadIdx.x; b < blockIdx.x; b += kCkThreads) {
        fin_before += block_sums[2 * b];
        units_before += block_sums[2 * b + 1];
    }
    fin_before = ckpt_block_sum(fin_before, scan);
    units_before = ckpt_block_sum(units_before, scan);
    uint8_t m[kCkPerThread];
    unsigned long long mine = 0;
    for(uint32_t k = 0; k < kCkPerThread; k++) {
        const uint32_t s = blockIdx.x * kCkPerBlock + threadIdx.x * kCkPerThread + k;
        m[k] = s < n_streams ? map[s] : (uint8_t)PT_CKPT_UNTOUCHED;
        mine += ((m[k] & 3u) == PT_CKPT_FINISHED ? 1ull : 0ull) + ((unsigned long long)ptd::ckpt_units(m[k]) << 32);
    }
    const unsigned long long incl = ckpt_block_scan(mine, scan);
    const unsigned long long block_total = scan[kCkThreads - 1];
    uint32_t fin = (uint32_t)(incl - mine), units = (uint32_t)((incl - mine) >> 32);
    for(uint32_t k = 0; k < kCkPerThread; k++) {
        const uint32_t ls = threadIdx.x * kCkPerThread + k, s = blockIdx.x * kCkPerBlock + ls;
        start[ls] = units;
        source[ls] = 0;
        if(s < n_streams) {
            const uint32_t tile = ptd::ckpt_stream_tile(s, tile_offset, n_tiles);
            if(tile_offset[tile] == s) {
                tile_finished[tile] = fin_before + fin;
                tile_units[tile] = units_before + units;
            }
            if((m[k] & 3u) == PT_CKPT_FINISHED) {
                if(out_records != nullptr && fin_before + fin < max_pixels) {
                    out_pixels[fin_before + fin] = image[ptd::ckpt_stream_pixel(s, tile, tiles, tile_offset, width)];
                }
                fin++;
            }
            else if((m[k] & 3u) == PT_CKPT_RECORD) {
                source[ls] = slot[s] - PT_CKPT_RECORD;
                units += ptd::ckpt_units(m[k]);
            }
        }
    }
    if(threadIdx.x == kCkThreads - 1) {
        start[kCkPerBlock] = (uint32_t)(block_total >> 32);
        if(blockIdx.x == gridDim.x - 1) {
            totals[PT_CKPT_TOTAL_FINISHED] = fin_before + (uint32_t)block_total;
            totals[PT_CKPT_TOTAL_UNITS] = units_before + (block_total >> 32);
        }
    }
    __syncthreads();
    if(out_records == nullptr) {
        return;
    }
    // one lane per unit of the workgroup's records: the last stream whose first unit is not behind it owns the unit
    const uint32_t n_units = start[kCkPerBlock];
    for(uint32_t u = threadIdx.x; u < n_units; u += kCkThreads) {
        uint32_t lo = 0, hi = kCkPerBlock;
        while(hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if(start[mid] <= u) {
                lo = mid;
            }
            else {
                hi = mid;
            }
        }
        if(units_before + u < max_units) {
            out_records[units_before + u] = ptd::ckpt_pack_unit(park + source[lo], u - start[lo]);
        }
    }
}

// ---- unpack -------------------------------------------------------------------------------------------------------------------------------

// Per workgroup of 1024 streams of the replica's map: streams with a record, untouched streams, record units (block_sums: [3 * workgroups])
__global__ __launch_bounds__(kCkThreads) void pt_checkpoint_count_kernel(const uint8_t *__restrict__ map, uint32_t n_streams, uint32_t *__restrict__ block_sums) {
    __shared__ unsigned long long red[kCkThreads];
    unsigned long long mine = 0;
    for(uint32_t k = 0; k < kCkPerThread; k++) {
        const uint32_t s = blockIdx.x * kCkPerBlock + threadIdx.x * kCkPerThread + k;
        if(s < n_streams) {
            const uint8_t m = map[s];
            mine += ((m & 3u) == PT_CKPT_RECORD ? 1ull : 0ull) + ((m & 3u) == PT_CKPT_UNTOUCHED ? 1ull << 21 : 0ull) + ((unsigned long long)ptd::ckpt_units(m) << 42);
        }
    }
    const unsigned long long sum = ckpt_block_sum(mine, red);
    if(threadIdx.x < 3) {
        block_sums[3 * blockIdx.x + threadIdx.x] = (uint32_t)((sum >> (21 * threadIdx.x)) & (threadIdx.x < 2 ? 0x1fffffull : ~0ull));
    }
}

// The work list (streams with a record first, in stream order, record r for the r-th of them; then the untouched streams in stream
// order), the full park records, and per workgroup the list's summary (partials: [PT_CKPT_PARTIALS * workgroups])
__global__ __launch_bounds__(kCkThreads) void pt_checkpoint_expand_kernel(const uint8_t *__restrict__ map, uint32_t n_streams, const uint32_t *__restrict__ block_sums,
                                                                          uint32_t n_blocks, const uint4 *__restrict__ trimmed, uint2 *__restrict__ todo,
                                                                          PtParkRecord *__restrict__ park, unsigned long long *__restrict__ partials) {
    __shared__ unsigned long long scan[kCkThreads];
    __shared__ uint32_t start[kCkPerBlock];  // record units of the workgroup before each of its streams
    __shared__ uint32_t owner[kCkPerBlock];  // the workgroup's r-th record belongs to this stream of it
    unsigned long long rec_before = 0, unt_before = 0, units_before = 0, rec_all = 0;
    for(uint32_t b = threadIdx.x; b < n_blocks; b += kCkThreads) {
        const uint32_t r = block_sums[3 * b];
        rec_all += r;
        if(b < blockIdx.x) {
            rec_before += r;
            unt_before += block_sums[3 * b + 1];
            units_before += block_sums[3 * b + 2];
        }
    }
    rec_all = ckpt_block_sum(rec_all, scan);
    rec_before = ckpt_block_sum(rec_before, scan);
    unt_before = ckpt_block_sum(unt_before, scan);
    units_before = ckpt_block_sum(units_before, scan);
    uint8_t m[kCkPerThread];
    unsigned long long mine = 0;
    for(uint32_t k = 0; k < kCkPerThread; k++) {
        const uint32_t s = blockIdx.x * kCkPerBlock + threadIdx.x * kCkPerThread + k;
        m[k] = s < n_streams ? map[s] : (uint8_t)PT_CKPT_FINISHED;
        mine += ((m[k] & 3u) == PT_CKPT_RECORD ? 1ull : 0ull) + ((m[k] & 3u) == PT_CKPT_UNTOUCHED ? 1ull << 21 : 0ull) + ((unsigned long long)ptd::ckpt_units(m[k]) << 42);
    }
    const unsigned long long incl = ckpt_block_scan(mine, scan);
    const uint32_t block_records = (uint32_t)(scan[kCkThreads - 1] & 0x1fffffull);
    const unsigned long long excl = incl - mine;
    uint32_t rec = (uint32_t)(excl & 0x1fffffull), unt = (uint32_t)((excl >> 21) & 0x1fffffull), units = (uint32_t)(excl >> 42);
    unsigned long long carried = 0, with_candidates = 0, least = 0xffffffffull, most = 0;
    for(uint32_t k = 0; k < kCkPerThread; k++) {
        const uint32_t ls = threadIdx.x * kCkPerThread + k, s = blockIdx.x * kCkPerBlock + ls;
        start[ls] = units;
        if(s >= n_streams || (m[k] & 3u) == PT_CKPT_FINISHED) {
            continue;
        }
        uint32_t samples = 0;
        if((m[k] & 3u) == PT_CKPT_RECORD) {
            const uint32_t r = (uint32_t)rec_before + rec;
            todo[r] = make_uint2(s, r);
            owner[rec] = ls;
            samples = (uint32_t)ptd::ckpt_samples(trimmed + units_before + units);
            with_candidates += (m[k] >> 2) != 0 ? 1ull : 0ull;
            rec++;
            units += ptd::ckpt_units(m[k]);
        }
        else {
            todo[(uint32_t)rec_all + (uint32_t)unt_before + unt] = make_uint2(s, PT_NO_PARK);
            unt++;
        }
        carried += samples;
        least = samples < least ? samples : least;
        most = samples > most ? samples : most;
    }
    // the summary, per workgroup: two sums, then a tree each for the least and the greatest sample count
    carried = ckpt_block_sum(carried, scan);
    with_candidates = ckpt_block_sum(with_candidates, scan);
    __syncthreads();
    scan[threadIdx.x] = least;
    __syncthreads();
    for(uint32_t d = kCkThreads / 2; d > 0; d >>= 1) {
        if(threadIdx.x < d) {
            scan[threadIdx.x] = scan[threadIdx.x + d] < scan[threadIdx.x] ? scan[threadIdx.x + d] : scan[threadIdx.x];
        }
        __syncthreads();
    }
    least = scan[0];
    __syncthreads();
    scan[threadIdx.x] = most;
    __syncthreads();
    for(uint32_t d = kCkThreads / 2; d > 0; d >>= 1) {
        if(threadIdx.x < d) {
            scan[threadIdx.x] = scan[threadIdx.x + d] > scan[threadIdx.x] ? scan[threadIdx.x + d] : scan[threadIdx.x];
        }
        __syncthreads();
    }
    most = scan[0];
    if(threadIdx.x == 0) {
        unsigned long long *p = partials + PT_CKPT_PARTIALS * blockIdx.x;
        p[PT_CKPT_CARRIED] = carried;
        p[PT_CKPT_WITH_CANDIDATES] = with_candidates;
        p[PT_CKPT_MIN] = least;
        p[PT_CKPT_MAX] = most;
    }
    __syncthreads();
    // one lane per unit of the workgroup's full records
    const uint32_t n_units = block_records * PT_CKPT_FULL_UNITS;
    for(uint32_t u = threadIdx.x; u < n_units; u += kCkThreads) {
        const uint32_t r = u / PT_CKPT_FULL_UNITS, j = u % PT_CKPT_FULL_UNITS, ls = owner[r];
        const uint8_t mb = map[blockIdx.x * kCkPerBlock + ls];
        reinterpret_cast<uint4 *>(park + (uint32_t)rec_before + r)[j] =
            ptd::ckpt_unpack_unit(trimmed + units_before + start[ls], (uint32_t)(mb >> 2) & 15u, blockIdx.x * kCkPerBlock + ls, j);
    }
}

} // namespace

#endif // PT_CHECKPOINT_HOST

#endif
