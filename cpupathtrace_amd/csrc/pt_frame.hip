// pt_frame.hip -- the work list of a resumable frame (pt_frame_render, pt_api.cpp).
//
// After a launch the frame's next work list is built from the status every stream of the launch left (PtStreams::status): finished
// streams leave the list, parked ones come first with their new park record, untouched ones follow without one.  Both parts keep the order
// of the old list (a stable partition in two kernels: counts per block of 1024 entries, then every block places its entries behind the
// counts of the blocks before it).  Parked streams first: the next launch's first round takes them all (it deals out at least as many
// streams as the launch before could park, one per slot), so no record has to outlive the launch that reads it.
#include <hip/hip_runtime.h>

#include "pt_kernels.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kPerThread = 4;
constexpr uint32_t kPerBlock = kThreads * kPerThread;

// what became of entry i: 0 = finished, 1 = parked in this launch, 2 = still to do from its seed
__device__ uint32_t entry_class(const uint2 *todo, const uint32_t *status, uint32_t i) {
    const uint32_t st = status[todo[i].x];
    return st == PT_STREAM_FINISHED ? 0u : (st >= PT_STREAM_PARKED ? 1u : 2u);
}

__global__ __launch_bounds__(kThreads) void pt_frame_count_kernel(const uint2 *__restrict__ todo, uint32_t n, const uint32_t *__restrict__ status,
                                                                  uint32_t *__restrict__ block_counts) {
    __shared__ uint32_t sum[2];
    if(threadIdx.x < 2) {
        sum[threadIdx.x] = 0;
    }
    __syncthreads();
    uint32_t parked = 0, fresh = 0;
    for(uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t i = blockIdx.x * kPerBlock + threadIdx.x * kPerThread + k;
        if(i < n) {
            const uint32_t c = entry_class(todo, status, i);
            parked += c == 1u ? 1u : 0u;
            fresh += c == 2u ? 1u : 0u;
        }
    }
    atomicAdd(&sum[0], parked);
    atomicAdd(&sum[1], fresh);
    __syncthreads();
    if(threadIdx.x < 2) {
        block_counts[2 * blockIdx.x + threadIdx.x] = sum[threadIdx.x];
    }
}

__global__ __launch_bounds__(kThreads) void pt_frame_place_kernel(const uint2 *__restrict__ todo, uint32_t n, uint32_t *__restrict__ status,
                                                                  const uint32_t *__restrict__ block_counts, uint32_t n_blocks, const PtParkRecord *__restrict__ parked,
                                                                  uint2 *__restrict__ todo_out, unsigned long long *__restrict__ result) {
    __shared__ uint32_t scan[kThreads];
    __shared__ uint32_t before[3]; // parked in earlier blocks, fresh in earlier blocks, parked in all blocks
    if(threadIdx.x < 3) {
        before[threadIdx.x] = 0;
    }
    __syncthreads();
    {
        uint32_t p_before = 0, f_before = 0, p_all = 0;
        for(uint32_t b = threadIdx.x; b < n_blocks; b += kThreads) {
            const uint32_t pb = block_counts[2 * b], fb = block_counts[2 * b + 1];
            p_all += pb;
            if(b < blockIdx.x) {
                p_before += pb;
                f_before += fb;
            }
        }
        atomicAdd(&before[0], p_before);
        atomicAdd(&before[1], f_before);
        atomicAdd(&before[2], p_all);
    }
    // the thread's entries, and an inclusive scan of (parked | fresh << 16) over the block's threads in thread order
    uint32_t cls[kPerThread];
    uint32_t mine = 0;
    for(uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t i = blockIdx.x * kPerBlock + threadIdx.x * kPerThread + k;
        cls[k] = i < n ? entry_class(todo, status, i) : 0u;
        mine += cls[k] == 1u ? 1u : (cls[k] == 2u ? 0x10000u : 0u);
    }
    scan[threadIdx.x] = mine;
    __syncthreads();
    for(uint32_t d = 1; d < kThreads; d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? scan[threadIdx.x - d] : 0u;
        __syncthreads();
        scan[threadIdx.x] += add;
        __syncthreads();
    }
    const uint32_t excl = scan[threadIdx.x] - mine;
    uint32_t at_parked = before[0] + (excl & 0xffffu);
    uint32_t at_fresh = before[2] + before[1] + (excl >> 16);
    uint32_t lost = 0, carried = 0, with_candidates = 0;
    for(uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t i = blockIdx.x * kPerBlock + threadIdx.x * kPerThread + k;
        if(i >= n || cls[k] == 0u) {
            continue;
        }
        const uint2 e = todo[i];
        if(cls[k] == 1u) {
            const uint32_t rec = status[e.x] - PT_STREAM_PARKED;
            todo_out[at_parked++] = make_uint2(e.x, rec);
            carried += (uint32_t)parked[rec].est.pixel_sample;
            with_candidates += parked[rec].est.n_candidates > 0 ? 1u : 0u;
        }
        else {
            // (a stream that held a record and was not taken this time starts afresh: the same bits, only its samples are lost)
            lost += e.y != PT_NO_PARK ? 1u : 0u;
            todo_out[at_fresh++] = make_uint2(e.x, PT_NO_PARK);
        }
        status[e.x] = PT_STREAM_UNTOUCHED; // (the status describes one launch)
    }
    if(lost != 0) {
        atomicAdd(&result[2], (unsigned long long)lost);
    }
    if(carried != 0) {
        atomicAdd(&result[3], (unsigned long long)carried);
    }
    if(with_candidates != 0) {
        atomicAdd(&result[4], (unsigned long long)with_candidates);
    }
    if(blockIdx.x == n_blocks - 1 && threadIdx.x == kThreads - 1) {
        result[0] = before[2];
        result[1] = before[1] + (scan[threadIdx.x] >> 16);
    }
}

} // namespace

int pt_launch_frame_compact(hipStream_t stream, const uint2 *todo, uint32_t n, uint32_t *status, const PtParkRecord *parked, uint2 *todo_out, uint32_t *block_counts,
                            unsigned long long *result) {
    if(hipMemsetAsync(result, 0, 8 * sizeof(unsigned long long), stream) != hipSuccess) {
        return 1;
    }
    if(n == 0) {
        return 0;
    }
    const uint32_t n_blocks = (n + kPerBlock - 1) / kPerBlock;
    pt_frame_count_kernel<<<n_blocks, kThreads, 0, stream>>>(todo, n, status, block_counts);
    pt_frame_place_kernel<<<n_blocks, kThreads, 0, stream>>>(todo, n, status, block_counts, n_blocks, parked, todo_out, result);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
