// pt_denoise.h -- the feature-guided a-trous denoiser (pt_denoise.hip): launch interface for the host side (pt_api.cpp).
#ifndef PT_DENOISE_H
#define PT_DENOISE_H

#include <hip/hip_runtime.h>

#include <cstdint>

struct PtDenoiseParams {
    int32_t iterations;
    float sigma_luminance, sigma_normal, sigma_depth;
};

// Device buffers of one denoise call, width * height entries each (the caller owns them).
struct PtDenoiseScratch {
    float4 *col[2];  // demodulated rgb, luminance (ping-pong)
    float *var[2];   // luminance variance (ping-pong)
    float4 *guide;   // normal xyz, mean hit distance
    float2 *grad;    // screen-space gradient of the hit distance
    uint32_t *cls;   // bit 0: some ray hit, bit 1: emissive
};

// Denoises `rgba` (width * height float4) guided by `features` (width * height * 3 float4, pt_render_features) into `out` (may equal rgba).
// Enqueues 3 + iterations launches on `stream` and returns the launch status; it does not wait.
hipError_t pt_denoise_run(hipStream_t stream, const float4 *rgba, const float4 *features, int32_t width, int32_t height, const PtDenoiseParams &params,
                          const PtDenoiseScratch &scratch, float4 *out);

#endif
