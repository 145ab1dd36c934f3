// pt_denoise.h -- the feature-guided a-trous denoiser (pt_denoise.hip): launch interface for the host side (pt_image.cpp,
// pt_frame_maps.cpp).
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

// pt_denoise_run with holes (pt_frame_preview): a pixel whose `samples` entry is 0 is a hole, never a tap of another pixel and filled from
// its own taps (pt_denoise.hip).  Without holes the result equals pt_denoise_run's bit for bit.  `out` may equal rgba.
hipError_t pt_denoise_masked_run(hipStream_t stream, const float4 *rgba, const float4 *features, const int32_t *samples, int32_t width, int32_t height,
                                 const PtDenoiseParams &params, const PtDenoiseScratch &scratch, float4 *out);

// A batch of n_views frames stacked as [n_views][height][width] (every array, the scratch buffers included, holds n_views * width * height
// pixels): view v comes out bit for bit as pt_denoise_run (samples == nullptr) or pt_denoise_masked_run gives on view v alone -- no tap
// crosses a view border.  3 + iterations launches for all views (the view is the grid's z; per 65535 views), n_views == 1 is the single
// frame's call itself.  `out` may equal rgba.
hipError_t pt_denoise_views_run(hipStream_t stream, const float4 *rgba, const float4 *features, const int32_t *samples, int32_t width, int32_t height,
                                int32_t n_views, const PtDenoiseParams &params, const PtDenoiseScratch &scratch, float4 *out);

// pt_denoise_run (samples == nullptr) or pt_denoise_masked_run with a plane of measured variances, `variance`: width * height float4
// (v_r, v_g, v_b, B), the variance of the mean of every channel of `rgba` and the batch means behind it (pt_frame_get_variance).  Where
// B >= 2 and every v_c is finite and not negative, the variance stage writes (0.2126 s_r + 0.7152 s_g + 0.0722 s_b)^2 with
// s_c = sqrtf(v_c) / max(albedo_c, 0.01) on the pixels prepare demodulates, sqrtf(v_c) elsewhere, in place of its 3x3 estimate, and the
// pixel's luminance sigma is sigma_measured.  A plane that rates no pixel gives the other run's result bit for bit.  `out` may equal rgba.
hipError_t pt_denoise_measured_run(hipStream_t stream, const float4 *rgba, const float4 *features, const float4 *variance, const int32_t *samples, int32_t width,
                                   int32_t height, const PtDenoiseParams &params, float sigma_measured, const PtDenoiseScratch &scratch, float4 *out);

// ---- the temporal form (pt_temporal_*): one push of a frame of a sequence ----------------------------------------------------------

struct PtTemporalParams {
    PtDenoiseParams spatial;
    float alpha_color, alpha_moments;
    int32_t max_history, moments_min_history;
    float sigma_luminance_temporal, normal_min, position_tolerance;
};

enum { PT_REPROJECT_NONE = 0, PT_REPROJECT_IDENTICAL = 1, PT_REPROJECT_CAMERA = 2 };

// Where the previous push's camera saw a point: X - origin = a forward + b up + c right, (a, b, c) = row . (X - origin) up to a positive
// factor (rows of the inverse of [forward up right], times |det|).  Derived on the host (pt_image.cpp).
struct PtReprojection {
    float origin[3];
    float row[3][3];
    float footprint; // the current camera's pixel footprint per unit hit distance: height / (focal_length * image height)
    int32_t mode;    // PT_REPROJECT_*: no previous push, the same camera bit for bit (each pixel is its own tap), another camera
};

// The device buffers of one temporal denoiser, width * height entries each; [cur] is written by this push, [cur ^ 1] holds the last one's.
struct PtTemporalState {
    float4 *col_hist;     // colour history: demodulated rgb + luminance after the first a-trous pass (read, then rewritten)
    float2 *moments[2];   // integrated luminance moments mu1, mu2
    int32_t *len[2];      // history length n (0 = no ray hit)
    float4 *pos[2];       // mean hit position
    float4 *nrm[2];       // mean normal
    uint32_t *cls[2];     // class (as PtDenoiseScratch::cls)
    int cur;
};

// One push: prepare, accumulate, variance, `iterations` a-trous launches (the first writes the colour history), finish.  scratch.cls is
// not used (state.cls[cur] is).  Enqueues on `stream` and returns the launch status; it does not wait.
hipError_t pt_temporal_run(hipStream_t stream, const float4 *rgba, const float4 *features, int32_t width, int32_t height, const PtTemporalParams &params,
                           const PtReprojection &reprojection, const PtDenoiseScratch &scratch, const PtTemporalState &state, float4 *out);

// pt_temporal_run with the frame's motion (width * height * 2 float4, pt_render_features_motion; include/pt_motion.h): the accumulate step
// reprojects where every pixel's surface was at the previous pose.  `reprojection` carries the previous camera's origin and rows in mode
// PT_REPROJECT_IDENTICAL too: a pixel on a moved surface is projected even under the same camera.
hipError_t pt_temporal_run_motion(hipStream_t stream, const float4 *rgba, const float4 *features, const float4 *motion, int32_t width, int32_t height,
                                  const PtTemporalParams &params, const PtReprojection &reprojection, const PtDenoiseScratch &scratch, const PtTemporalState &state,
                                  float4 *out);

#endif
