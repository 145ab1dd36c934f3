// TEST ONLY: the host stand-in for the HIP runtime (tests/hip/host) with what tests/hip/deform_probe.hip and the skinning kernel
// (pt_deform_kernels.h) need on top of it: block-shared memory and ONE barrier per kernel.  A launch runs every block twice: in the
// first pass each thread runs up to the barrier and leaves there, so that the whole block has staged its part of the shared array; in
// the second pass the barrier lets every thread through (what it staged before, it stages again, with the same values).  A kernel that
// let a thread return before the barrier, or that computed from the shared array before it, would read entries that nobody has written.
// tests/deform_probe.py compiles the probe against this directory.
#pragma once
#include "../../host/hip/hip_runtime.h"
enum { hipErrorInvalidValue = 1 };
#ifndef __restrict__
#define __restrict__ __restrict
#endif
#define __shared__ static
struct ShimBarrier {};
inline thread_local int shim_pass = 1;
inline void __syncthreads() {
    if(shim_pass == 0) {
        throw ShimBarrier{};
    }
}
template<typename F> void shim_launch_block_twice(dim3 g, dim3 b, F f) {
    for(unsigned gx = 0; gx < g.x; gx++) {
        for(shim_pass = 0; shim_pass < 2; shim_pass++) {
            for(unsigned tx = 0; tx < b.x; tx++) {
                blockIdx = dim3(gx, 0, 0);
                threadIdx = dim3(tx, 0, 0);
                try {
                    f();
                }
                catch(const ShimBarrier &) {
                }
            }
        }
    }
    shim_pass = 1;
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) shim_launch_block_twice(g, b, [&] { k(__VA_ARGS__); })
