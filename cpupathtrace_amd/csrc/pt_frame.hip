// pt_frame.hip -- the work list of a resumable frame (pt_frame_render, pt_frames.cpp).
//
// After a launch the frame's next work list is built from the status every stream of the launch left (PtStreams::status): finished
// streams leave the list, parked ones come first with their new park record, untouched ones follow without one.  Both parts keep the order
// of the old list (a stable partition in two kernels: counts per block of 1024 entries, then every block places its entries behind the
// counts of the blocks before it).  Parked streams first: the next launch's first round takes them all (it deals out at least as many
// streams as the launch before could park, one per slot), so no record has to outlive the launch that reads it.
//
//
// A progressive frame (pt_frame_set_progressive) renders in passes: every stream parks when its pixel has the pass's sample count `target`
// (PtStreams::yield_at), so a launch leaves up to one record per entry of its list.  Its list is split by sample count instead: streams
// below the target first (what an interrupted pass has left to do), streams at it behind them, each part in the order of the old list.  An
// entry the launch never claimed keeps its record: the carry kernel copies it from the launch's input records to its output records, behind
// the ones the launch wrote, so no sample is ever lost.
//
// A progressive frame with a noise target (pt_frame_set_noise_target; PtNoiseRule::target > 0) has a third part behind those two: the HELD
// streams, whose pixel is rated (pixel_error, pt_noise.h) at or below the target.  A pass's launch takes the list without that part, so a
// held stream is never claimed and its record is carried like any unclaimed one.  Whether a stream is held is read from its record every
// time a list is built and stored nowhere.  Before a pass the host has the list built once more with nothing launched (`resort`): every
// record stays where it is and only the list is split again, by the pass's sample count and the target as they are now.
//
// The same work list is what pt_frame_preview shows between two launches: the gather kernels below read it without changing it, and
// pt_frame_rate_kernel rates its pixels for pt_frame_get_noise, pt_frame_variance_kernel gives their measured variance for
// pt_frame_get_variance.
#include <hip/hip_runtime.h>

#include "pt_kernels.h"
#include "pt_noise.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kPerThread = 4;
constexpr uint32_t kPerBlock = kThreads * kPerThread;

// a record of the launch's INPUT buffer that the carry kernel has yet to move: bit 31 of a work-list entry's y (a record index has 28 bits)
constexpr uint32_t kCarry = 0x80000000u;

// what became of entry i (PtEntryClass): finished, FIRST = parked in this launch, SECOND = still to do from its seed.  In a progressive
// frame (target > 0): finished, FIRST = its pixel has fewer than `target` samples, SECOND = it has them; `samples` is that count and `where`
// (PtEntryRecord) says where the stream's record, index `rec`, is: it has none, the launch wrote it, or it was never claimed.  With a noise
// target, HELD: the stream has a record and its pixel's error is at or below the target (an unrated pixel's is +inf).
__device__ uint32_t entry_class(const uint2 *todo, const uint32_t *status, uint32_t i, int32_t target, const PtParkRecord *parked, const PtParkRecord *park_in,
                                const PtNoiseRule &noise, uint32_t &where, uint32_t &rec, int32_t &samples) {
    const uint2 e = todo[i];
    const uint32_t st = status[e.x];
    where = PT_RECORD_NONE;
    rec = PT_NO_PARK;
    samples = 0;
    if(target <= 0) {
        return st == PT_STREAM_FINISHED ? PT_ENTRY_FINISHED : (st >= PT_STREAM_PARKED ? PT_ENTRY_FIRST : PT_ENTRY_SECOND);
    }
    if(st == PT_STREAM_FINISHED) {
        return PT_ENTRY_FINISHED;
    }
    if(st >= PT_STREAM_PARKED) {
        where = PT_RECORD_WRITTEN;
        rec = st - PT_STREAM_PARKED;
        samples = parked[rec].est.pixel_sample;
    }
    else if(e.y != PT_NO_PARK) {
        where = PT_RECORD_UNCLAIMED;
        rec = e.y;
        samples = park_in[rec].est.pixel_sample;
    }
    if(noise.target > 0.0f && where != PT_RECORD_NONE && pixel_error((where == PT_RECORD_WRITTEN ? parked : park_in)[rec].est, noise.opt, noise.floor) <= noise.target) {
        return PT_ENTRY_HELD;
    }
    return samples < target ? PT_ENTRY_FIRST : PT_ENTRY_SECOND;
}

__global__ __launch_bounds__(kThreads) void pt_frame_count_kernel(const uint2 *__restrict__ todo, uint32_t n, const uint32_t *__restrict__ status,
                                                                  uint32_t *__restrict__ block_counts, int32_t target, const PtParkRecord *__restrict__ parked,
                                                                  const PtParkRecord *__restrict__ park_in, PtNoiseRule noise) {
    __shared__ uint32_t sum[3];
    if(threadIdx.x < 3) {
        sum[threadIdx.x] = 0;
    }
    __syncthreads();
    uint32_t first = 0, second = 0, third = 0;
    for(uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t i = blockIdx.x * kPerBlock + threadIdx.x * kPerThread + k;
        if(i < n) {
            uint32_t where, rec;
            int32_t samples;
            const uint32_t c = entry_class(todo, status, i, target, parked, park_in, noise, where, rec, samples);
            first += c == PT_ENTRY_FIRST ? 1u : 0u;
            second += c == PT_ENTRY_SECOND ? 1u : 0u;
            third += c == PT_ENTRY_HELD ? 1u : 0u;
        }
    }
    atomicAdd(&sum[0], first);
    atomicAdd(&sum[1], second);
    if(third != 0) {
        atomicAdd(&sum[2], third);
    }
    __syncthreads();
    if(threadIdx.x < 3) {
        block_counts[3 * blockIdx.x + threadIdx.x] = sum[threadIdx.x];
    }
}

__global__ __launch_bounds__(kThreads) void pt_frame_place_kernel(const uint2 *__restrict__ todo, uint32_t n, uint32_t *__restrict__ status,
                                                                  const uint32_t *__restrict__ block_counts, uint32_t n_blocks, const PtParkRecord *__restrict__ parked,
                                                                  uint2 *__restrict__ todo_out, unsigned long long *__restrict__ result, int32_t target,
                                                                  const PtParkRecord *__restrict__ park_in, PtNoiseRule noise, int resort) {
    __shared__ unsigned long long scan[kThreads];
    // first class in earlier blocks, second class in earlier blocks, first class in all blocks, held in earlier blocks, second class in all blocks
    __shared__ uint32_t before[5];
    if(threadIdx.x < 5) {
        before[threadIdx.x] = 0;
    }
    __syncthreads();
    {
        uint32_t p_before = 0, f_before = 0, p_all = 0, h_before = 0, f_all = 0;
        for(uint32_t b = threadIdx.x; b < n_blocks; b += kThreads) {
            const uint32_t pb = block_counts[3 * b], fb = block_counts[3 * b + 1];
            p_all += pb;
            f_all += fb;
            if(b < blockIdx.x) {
                p_before += pb;
                f_before += fb;
                h_before += block_counts[3 * b + 2];
            }
        }
        atomicAdd(&before[0], p_before);
        atomicAdd(&before[1], f_before);
        atomicAdd(&before[2], p_all);
        atomicAdd(&before[3], h_before);
        atomicAdd(&before[4], f_all);
    }
    // the thread's entries, and an inclusive scan of (first class | second class << 21 | held << 42) over the block's threads in thread order
    uint32_t cls[kPerThread], where[kPerThread], rec[kPerThread];
    int32_t samples[kPerThread];
    unsigned long long mine = 0;
    for(uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t i = blockIdx.x * kPerBlock + threadIdx.x * kPerThread + k;
        where[k] = PT_RECORD_NONE;
        rec[k] = PT_NO_PARK;
        samples[k] = 0;
        cls[k] = i < n ? entry_class(todo, status, i, target, parked, park_in, noise, where[k], rec[k], samples[k]) : PT_ENTRY_FINISHED;
        mine += cls[k] == PT_ENTRY_FIRST ? 1ull : (cls[k] == PT_ENTRY_SECOND ? 1ull << 21 : (cls[k] == PT_ENTRY_HELD ? 1ull << 42 : 0ull));
    }
    scan[threadIdx.x] = mine;
    __syncthreads();
    for(uint32_t d = 1; d < kThreads; d <<= 1) {
        const unsigned long long add = threadIdx.x >= d ? scan[threadIdx.x - d] : 0ull;
        __syncthreads();
        scan[threadIdx.x] += add;
        __syncthreads();
    }
    const unsigned long long excl = scan[threadIdx.x] - mine;
    uint32_t at_first = before[0] + (uint32_t)(excl & 0x1fffffu);
    uint32_t at_second = before[2] + before[1] + (uint32_t)((excl >> 21) & 0x1fffffu);
    uint32_t at_held = before[2] + before[4] + before[3] + (uint32_t)(excl >> 42);
    uint32_t lost = 0, carried = 0, with_candidates = 0, with_record = 0, written = 0, least = 0xffffffffu, most = 0;
    for(uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t i = blockIdx.x * kPerBlock + threadIdx.x * kPerThread + k;
        if(i >= n || cls[k] == PT_ENTRY_FINISHED) {
            continue;
        }
        const uint2 e = todo[i];
        uint32_t s = 0; // samples the pixel has taken
        if(target > 0) {
            // a progressive frame: the record stays with the stream wherever it is (an unclaimed one is moved by the carry kernel,
            // unless the list is only split again: then the input records stay the frame's records)
            const uint32_t y = where[k] == PT_RECORD_WRITTEN ? rec[k] : (where[k] == PT_RECORD_UNCLAIMED ? (resort != 0 ? rec[k] : (rec[k] | kCarry)) : PT_NO_PARK);
            if(cls[k] == PT_ENTRY_FIRST) {
                todo_out[at_first++] = make_uint2(e.x, y);
            }
            else if(cls[k] == PT_ENTRY_SECOND) {
                todo_out[at_second++] = make_uint2(e.x, y);
            }
            else {
                todo_out[at_held++] = make_uint2(e.x, y);
            }
            s = (uint32_t)samples[k];
            if(where[k] != PT_RECORD_NONE) {
                with_record++;
                written += where[k] == PT_RECORD_WRITTEN ? 1u : 0u;
                with_candidates += (where[k] == PT_RECORD_WRITTEN ? parked[rec[k]] : park_in[rec[k]]).est.n_candidates > 0 ? 1u : 0u;
            }
        }
        else if(cls[k] == PT_ENTRY_FIRST) {
            const uint32_t r = status[e.x] - PT_STREAM_PARKED;
            todo_out[at_first++] = make_uint2(e.x, r);
            s = (uint32_t)parked[r].est.pixel_sample;
            with_candidates += parked[r].est.n_candidates > 0 ? 1u : 0u;
            with_record++;
            written++;
        }
        else {
            // (a stream that held a record and was not taken this time starts afresh: the same bits, only its samples are lost)
            lost += e.y != PT_NO_PARK ? 1u : 0u;
            todo_out[at_second++] = make_uint2(e.x, PT_NO_PARK);
        }
        carried += s;
        least = s < least ? s : least;
        most = s > most ? s : most;
        status[e.x] = PT_STREAM_UNTOUCHED; // (the status describes one launch)
    }
    if(lost != 0) {
        atomicAdd(&result[PT_COMPACT_LOST], (unsigned long long)lost);
    }
    if(carried != 0) {
        atomicAdd(&result[PT_COMPACT_CARRIED], (unsigned long long)carried);
    }
    if(with_candidates != 0) {
        atomicAdd(&result[PT_COMPACT_WITH_CANDIDATES], (unsigned long long)with_candidates);
    }
    if(least != 0xffffffffu) {
        atomicMax(&result[PT_COMPACT_MIN_INVERTED], (unsigned long long)(0xffffffffu - least)); // (a minimum over a word that starts at zero)
        atomicMax(&result[PT_COMPACT_MAX], (unsigned long long)most);
    }
    if(with_record != 0) {
        atomicAdd(&result[PT_COMPACT_WITH_RECORD], (unsigned long long)with_record);
    }
    if(written != 0) {
        atomicAdd(&result[PT_COMPACT_WRITTEN], (unsigned long long)written);
    }
    if(blockIdx.x == n_blocks - 1 && threadIdx.x == kThreads - 1) {
        result[PT_COMPACT_FIRST] = before[2];
        result[PT_COMPACT_SECOND] = before[4];
        result[PT_COMPACT_HELD] = before[3] + (uint32_t)(scan[threadIdx.x] >> 42);
    }
}

// A progressive frame: the records of the entries the launch never claimed, from its input records to its output records.  A wavefront
// takes kCarryPerWave entries of the new work list one after the other; a record is 33 x 16 bytes, copied by 33 neighbouring lanes.  The
// record's new place is the next free one behind those the launch wrote (park_count goes on counting).  result[PT_COMPACT_NO_ROOM]
// counts the samples of records that found no room (none: the host sizes the output for every entry of the list).
constexpr uint32_t kCarryPerWave = 16;
static_assert(sizeof(PtParkRecord) == 33 * sizeof(uint4), "a park record is 33 x 16 bytes");

__global__ __launch_bounds__(kThreads) void pt_frame_carry_kernel(uint2 *__restrict__ todo_out, const PtParkRecord *__restrict__ park_in, PtParkRecord *__restrict__ park_out,
                                                                  uint32_t *__restrict__ park_count, uint32_t park_cap, unsigned long long *__restrict__ result) {
    const uint32_t n = (uint32_t)(result[PT_COMPACT_FIRST] + result[PT_COMPACT_SECOND] + result[PT_COMPACT_HELD]); // (the new list's length, left by the place kernel)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * kThreads + threadIdx.x) / 64u;
    for(uint32_t k = 0; k < kCarryPerWave; k++) {
        const uint32_t i = wave * kCarryPerWave + k;
        if(i >= n) {
            return;
        }
        const uint2 e = todo_out[i];
        if(e.y == PT_NO_PARK || (e.y & kCarry) == 0u) {
            continue;
        }
        const uint32_t src = e.y & ~kCarry;
        uint32_t dst = 0;
        if(lane == 0) {
            dst = atomicAdd(park_count, 1u);
        }
        dst = (uint32_t)__shfl((int)dst, 0);
        if(dst < park_cap) {
            if(lane < 33u) {
                reinterpret_cast<uint4 *>(park_out + dst)[lane] = reinterpret_cast<const uint4 *>(park_in + src)[lane];
            }
            if(lane == 0) {
                todo_out[i].y = dst;
            }
        }
        else if(lane == 0) {
            todo_out[i].y = PT_NO_PARK;
            atomicAdd(&result[PT_COMPACT_NO_ROOM], (unsigned long long)park_in[src].est.pixel_sample);
        }
    }
}

// ---- the preview of a frame (pt_frame_preview, pt_frame_maps.cpp) -----------------------------------------------------------------------
// Each replica gathers its work list into compact entries (gather); replica 0's device lays the frame out from the caller's image (base)
// and writes every replica's entries over it (scatter).

// The pixel of stream `stream` of a replica, as tile_stream (pt_path.hip) finds it: the last tile whose first stream is not behind it
__device__ int32_t stream_pixel(uint32_t stream, const int4 *tiles, const uint32_t *tile_offset, uint32_t n_tiles, int32_t width) {
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
    const int4 t = tiles[lo];
    const uint32_t k = stream - tile_offset[lo];
    const int32_t x = t.x + (int32_t)(k % (uint32_t)t.z), y = t.y + (int32_t)(k / (uint32_t)t.z);
    return y * width + x;
}

// One thread per entry of a replica's work list todo[0 .. n): an entry that names a record is a parked stream with its record in `park`
// (the first n_parked entries of a plain frame's list; any entry of a progressive frame's), the others are untouched.  Writes the entry's preview colour and (pixel, samples): the running mean pixel_value * (1 / collected_sample_count) and
// pixel_sample of a parked stream (estimator_finish's first step, pt_shading.h), (0, 0, 0, 0) and 0 samples for an untouched one.  A parked
// entry reads three fields of its 528-byte record, not the record.
__global__ __launch_bounds__(kThreads) void pt_frame_gather_kernel(const uint2 *__restrict__ todo, uint32_t n, uint32_t n_parked,
                                                                   const PtParkRecord *__restrict__ park, const int4 *__restrict__ tiles,
                                                                   const uint32_t *__restrict__ tile_offset, uint32_t n_tiles, int32_t width,
                                                                   float4 *__restrict__ out_rgba, int2 *__restrict__ out_at) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if(i >= n) {
        return;
    }
    const uint2 e = todo[i];
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int32_t samples = 0;
    if(e.y != PT_NO_PARK) {
        const PtEstimator &est = park[e.y].est;
        const float4 pv = *reinterpret_cast<const float4 *>(est.pixel_value);
        const int32_t collected = est.collected_sample_count;
        samples = est.pixel_sample;
        if(collected > 0) {
            const float inv = 1.0f / (float)collected;
            c = make_float4(pv.x * inv, pv.y * inv, pv.z * inv, pv.w * inv);
        }
    }
    out_rgba[i] = c;
    out_at[i] = make_int2(stream_pixel(e.x, tiles, tile_offset, n_tiles, width), samples);
}

// One thread per pixel: a pixel of some tile keeps the caller's colour and is finished (-1) until a scatter says otherwise; a pixel of
// no tile is a hole.
__global__ __launch_bounds__(kThreads) void pt_frame_preview_base_kernel(float4 *__restrict__ view, int32_t *__restrict__ samples,
                                                                         const uint8_t *__restrict__ cover, uint32_t n_pixels) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if(p >= n_pixels) {
        return;
    }
    if(cover[p] != 0) {
        samples[p] = -1;
    }
    else {
        view[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        samples[p] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void pt_frame_scatter_kernel(const float4 *__restrict__ rgba, const int2 *__restrict__ at, uint32_t n,
                                                                    float4 *__restrict__ view, int32_t *__restrict__ samples) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if(i >= n) {
        return;
    }
    const int2 a = at[i];
    view[a.x] = rgba[i];
    samples[a.x] = a.y;
}

// ---- the rating of a frame (pt_frame_get_noise, pt_frame_maps.cpp) ----------------------------------------------------------------------
// One thread per entry of a replica's work list, as the gather kernel: out[i] = (pixel, bits of its error), +inf for an entry without a
// record or with fewer than two batch means (unrated).  Reads the estimator's fields pixel_error needs, not the record.  The summary is
// reduced with integer atomics only, per block in LDS and then once per block (PtNoiseWord; errors are never negative, so their bits order as
// they do; a NaN error, 0 / 0 at floor 0, has the pattern 0xffc00000 here, which is above every number's: it becomes the maximum and
// lands in bin 63).
__global__ __launch_bounds__(kThreads) void pt_frame_rate_kernel(const uint2 *__restrict__ todo, uint32_t n, const PtParkRecord *__restrict__ park,
                                                                 const int4 *__restrict__ tiles, const uint32_t *__restrict__ tile_offset, uint32_t n_tiles,
                                                                 int32_t width, PtNoiseRule noise, uint2 *__restrict__ out, uint32_t *__restrict__ summary) {
    __shared__ uint32_t part[PT_NOISE_SUMMARY_WORDS];
    if(threadIdx.x < PT_NOISE_SUMMARY_WORDS) {
        part[threadIdx.x] = 0;
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if(i < n) {
        const uint2 e = todo[i];
        float error = __builtin_inff();
        bool rated = false;
        if(e.y != PT_NO_PARK) {
            const PtEstimator &est = park[e.y].est;
            rated = pixel_batches(est, noise.opt) >= 2;
            error = pixel_error(est, noise.opt, noise.floor);
        }
        out[i] = make_uint2((uint32_t)stream_pixel(e.x, tiles, tile_offset, n_tiles, width), __float_as_uint(error));
        if(rated) {
            atomicAdd(&part[PT_NOISE_RATED], 1u);
            if(noise.target > 0.0f && error <= noise.target) {
                atomicAdd(&part[PT_NOISE_HELD], 1u);
            }
            atomicMax(&part[PT_NOISE_MAX_BITS], __float_as_uint(error));
            atomicAdd(&part[PT_NOISE_FIRST_BIN + pixel_error_bin(error)], 1u);
        }
        else {
            atomicAdd(&part[PT_NOISE_UNRATED], 1u);
        }
    }
    __syncthreads();
    if(threadIdx.x < PT_NOISE_SUMMARY_WORDS && part[threadIdx.x] != 0) {
        if(threadIdx.x == PT_NOISE_MAX_BITS) {
            atomicMax(&summary[PT_NOISE_MAX_BITS], part[PT_NOISE_MAX_BITS]);
        }
        else {
            atomicAdd(&summary[threadIdx.x], part[threadIdx.x]);
        }
    }
}

// The error map on replica 0's device, one thread per pixel: -1 (finished) where a tile of a replica that has rendered covers the pixel,
// until a scatter says otherwise; +inf elsewhere.
__global__ __launch_bounds__(kThreads) void pt_frame_noise_base_kernel(float *__restrict__ map, const uint8_t *__restrict__ cover, uint32_t n_pixels) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if(p < n_pixels) {
        map[p] = cover[p] != 0 ? -1.0f : __builtin_inff();
    }
}

__global__ __launch_bounds__(kThreads) void pt_frame_noise_scatter_kernel(const uint2 *__restrict__ rated, uint32_t n, float *__restrict__ map) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if(i < n) {
        const uint2 a = rated[i];
        map[a.x] = __uint_as_float(a.y);
    }
}

// ---- the variance map of a frame (pt_frame_get_variance, pt_frame_maps.cpp) -------------------------------------------------------------
// One thread per entry of a replica's work list, as the rating kernel: out_var[i] = pixel_variance of the entry's record, (0, 0, 0, 0)
// for an entry without one, and out_at[i] its pixel.  Reads the estimator's M2 and sample count, not the record.
__global__ __launch_bounds__(kThreads) void pt_frame_variance_kernel(const uint2 *__restrict__ todo, uint32_t n, const PtParkRecord *__restrict__ park,
                                                                     const int4 *__restrict__ tiles, const uint32_t *__restrict__ tile_offset, uint32_t n_tiles,
                                                                     int32_t width, PtDevOptions opt, float4 *__restrict__ out_var, int32_t *__restrict__ out_at) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if(i >= n) {
        return;
    }
    const uint2 e = todo[i];
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if(e.y != PT_NO_PARK) {
        v = pixel_variance(park[e.y].est, opt);
    }
    out_var[i] = v;
    out_at[i] = stream_pixel(e.x, tiles, tile_offset, n_tiles, width);
}

// (the map on replica 0's device starts as zeros: finished, untouched and uncovered pixels stay (0, 0, 0, 0))
__global__ __launch_bounds__(kThreads) void pt_frame_variance_scatter_kernel(const float4 *__restrict__ var, const int32_t *__restrict__ at, uint32_t n,
                                                                             float4 *__restrict__ map) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if(i < n) {
        map[at[i]] = var[i];
    }
}

// One thread per item: the launch of every kernel above that takes its items one by one.  0, or 1 when the launch failed.
template<typename Kernel, typename... Args>
int launch_per_item(Kernel kernel, uint32_t n, hipStream_t stream, Args... args) {
    if(n == 0) {
        return 0;
    }
    kernel<<<(n + kThreads - 1) / kThreads, kThreads, 0, stream>>>(args...);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace

int pt_launch_frame_rate(hipStream_t stream, const uint2 *todo, uint32_t n, const PtParkRecord *park, const int4 *tiles, const uint32_t *tile_offset, uint32_t n_tiles,
                         int32_t width, const PtNoiseRule &noise, uint2 *out, uint32_t *summary) {
    if(hipMemsetAsync(summary, 0, PT_NOISE_SUMMARY_WORDS * sizeof(uint32_t), stream) != hipSuccess) {
        return 1;
    }
    return launch_per_item(pt_frame_rate_kernel, n, stream, todo, n, park, tiles, tile_offset, n_tiles, width, noise, out, summary);
}

int pt_launch_frame_noise_base(hipStream_t stream, float *map, const uint8_t *cover, uint32_t n_pixels) {
    return launch_per_item(pt_frame_noise_base_kernel, n_pixels, stream, map, cover, n_pixels);
}

int pt_launch_frame_noise_scatter(hipStream_t stream, const uint2 *rated, uint32_t n, float *map) {
    return launch_per_item(pt_frame_noise_scatter_kernel, n, stream, rated, n, map);
}

int pt_launch_frame_compact(hipStream_t stream, const uint2 *todo, uint32_t n, uint32_t *status, const PtParkRecord *parked, uint2 *todo_out, uint32_t *block_counts,
                            unsigned long long *result, int32_t target, const PtParkRecord *park_in, PtParkRecord *park_out, uint32_t *park_count, uint32_t park_cap,
                            const PtNoiseRule &noise, int resort) {
    if(hipMemsetAsync(result, 0, PT_COMPACT_WORDS * sizeof(unsigned long long), stream) != hipSuccess) {
        return 1;
    }
    if(n == 0) {
        return 0;
    }
    const uint32_t n_blocks = (n + kPerBlock - 1) / kPerBlock;
    pt_frame_count_kernel<<<n_blocks, kThreads, 0, stream>>>(todo, n, status, block_counts, target, parked, park_in, noise);
    pt_frame_place_kernel<<<n_blocks, kThreads, 0, stream>>>(todo, n, status, block_counts, n_blocks, parked, todo_out, result, target, park_in, noise, resort);
    if(target > 0 && resort == 0) {
        const uint32_t per_block = (kThreads / 64u) * kCarryPerWave;
        pt_frame_carry_kernel<<<(n + per_block - 1) / per_block, kThreads, 0, stream>>>(todo_out, park_in, park_out, park_count, park_cap, result);
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int pt_launch_frame_gather(hipStream_t stream, const uint2 *todo, uint32_t n, uint32_t n_parked, const PtParkRecord *park, const int4 *tiles,
                           const uint32_t *tile_offset, uint32_t n_tiles, int32_t width, float4 *out_rgba, int2 *out_at) {
    return launch_per_item(pt_frame_gather_kernel, n, stream, todo, n, n_parked, park, tiles, tile_offset, n_tiles, width, out_rgba, out_at);
}

int pt_launch_frame_preview_base(hipStream_t stream, float4 *view, int32_t *samples, const uint8_t *cover, uint32_t n_pixels) {
    return launch_per_item(pt_frame_preview_base_kernel, n_pixels, stream, view, samples, cover, n_pixels);
}

int pt_launch_frame_scatter(hipStream_t stream, const float4 *rgba, const int2 *at, uint32_t n, float4 *view, int32_t *samples) {
    return launch_per_item(pt_frame_scatter_kernel, n, stream, rgba, at, n, view, samples);
}

int pt_launch_frame_variance(hipStream_t stream, const uint2 *todo, uint32_t n, const PtParkRecord *park, const int4 *tiles, const uint32_t *tile_offset,
                             uint32_t n_tiles, int32_t width, const PtDevOptions &opt, float4 *out_var, int32_t *out_at) {
    return launch_per_item(pt_frame_variance_kernel, n, stream, todo, n, park, tiles, tile_offset, n_tiles, width, opt, out_var, out_at);
}

int pt_launch_frame_variance_scatter(hipStream_t stream, const float4 *var, const int32_t *at, uint32_t n, float4 *map) {
    return launch_per_item(pt_frame_variance_scatter_kernel, n, stream, var, at, n, map);
}
