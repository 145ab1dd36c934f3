// TEST ONLY: the host stand-in for the HIP runtime (tests/hip/host) with what tests/hip/query_probe.hip and the device functions it
// compiles for the host (pt_device.h, pt_kernels.h, pt_query_kernels.h) need on top of it: the integer vector types and the bit casts.
// tests/test_query_cpu.py compiles the probe against this directory.
#pragma once
#include "../../host/hip/hip_runtime.h"
struct uint2 { unsigned x, y; };
struct int2 { int x, y; };
struct alignas(16) uint4 { unsigned x, y, z, w; };
struct alignas(16) int4 { int x, y, z, w; };
inline uint2 make_uint2(unsigned x, unsigned y) { return uint2{x, y}; }
inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
inline float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
#ifndef __restrict__
#define __restrict__ __restrict
#endif
