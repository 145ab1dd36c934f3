// TEST ONLY: a host stand-in for the HIP runtime, enough of it for tests/hip/denoise_probe.hip and pt_denoise.hip.  A kernel launch runs the
// kernel as plain C++ loops over grid and block, device memory is host memory.  tests/denoise_probe.py: build_host() compiles the probe
// against it, so that the kernels' own source, guard bands included, runs where there is no GPU (with the C library's expf and powf).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <cstddef>
struct float2 { float x, y; };
struct alignas(16) float4 { float x, y, z, w; };
inline float2 make_float2(float x, float y) { return float2{x, y}; }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
inline thread_local dim3 blockIdx, threadIdx;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
typedef int hipError_t;
typedef void *hipStream_t;
enum { hipSuccess = 0 };
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipMalloc(void **p, size_t n) { *p = aligned_alloc(64, (n + 63) / 64 * 64); return *p ? 0 : 2; }
inline hipError_t hipFree(void *p) { free(p); return 0; }
inline hipError_t hipMemset(void *p, int v, size_t n) { memset(p, v, n); return 0; }
inline hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return 0; }
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return 0; }
inline hipError_t hipSetDevice(int) { return 0; }
inline hipError_t hipStreamCreate(hipStream_t *s) { *s = (void *)1; return 0; }
inline hipError_t hipStreamDestroy(hipStream_t) { return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
inline hipError_t hipGetDeviceCount(int *n) { *n = 1; return 0; }
inline const char *hipGetErrorString(hipError_t) { return "host"; }
inline int max(int a, int b) { return a > b ? a : b; }
inline int min(int a, int b) { return a < b ? a : b; }
template<typename F> void shim_launch(dim3 g, dim3 b, F f) {
    for(unsigned gz = 0; gz < g.z; gz++) for(unsigned gy = 0; gy < g.y; gy++) for(unsigned gx = 0; gx < g.x; gx++)
        for(unsigned ty = 0; ty < b.y; ty++) for(unsigned tx = 0; tx < b.x; tx++) {
            blockIdx = dim3(gx, gy, gz); threadIdx = dim3(tx, ty, 0); f();
        }
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) shim_launch(g, b, [&] { k(__VA_ARGS__); })
