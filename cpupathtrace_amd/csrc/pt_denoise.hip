// pt_denoise.hip -- feature-guided denoising of a finished frame (RenderOptions::allow_bias): the spatial part of SVGF (Schied et al. 2017)
// on the features of pt_feature_kernel (pt_walks.hip).  DESIGN.md 4.10 has the algorithm, its constants and its measured cost;
// tests/denoise_ref.py restates every kernel below in numpy, operation for operation.
//
//   prepare   c = rgb / max(albedo, 0.01) on covered, non-emissive pixels (rgb elsewhere), its luminance, the guide (n, t), the class
//   variance  the hit distance's screen-space gradient and the luminance variance over the edge-aware 3x3 neighbourhood
//   atrous    one pass of the 5x5 B3-spline kernel at step 2^i with normal, depth and luminance weights (variance: squared weights)
//   finish    rgb = c * the factor of `prepare`, alpha copied from the input
//
// pt_temporal_run, the temporal half of SVGF (tests/temporal_ref.py), adds one step between prepare and variance:
//   accumulate  reproject each covered pixel into the previous push's camera, blend the history of the bilinear taps that see the same
//               surface into c and into the luminance moments
// and runs variance and atrous in their kTemporal form: the moments' variance and sigma_luminance_temporal where the history is long enough.
//
// pt_denoise_masked_run, the preview of an unfinished frame (pt_frame_preview; tests/preview_ref.py), runs prepare,
// variance, atrous and finish in their kMasked form: a pixel without samples is a HOLE (class bit PTDN_HOLE, colour 0).  A hole is of
// another class than every pixel but holes, so it is never a tap; the 3x3 prefilter of the variance skips it too.  In every a-trous pass a
// hole takes the normalised weighted mean of the taps of its own class that are not holes (its own weight 0, no luminance term: the normal
// and depth terms of a covered hole, the B3 weights alone for an uncovered one), or keeps its value when no such tap has weight.  A hole's
// variance is read by no other pixel: it records whether a pass has filled the hole (1) or not (0).  Without holes every kMasked kernel
// computes what its plain form does, operation for operation.
//
// pt_denoise_views_run, a batch of V frames stacked as [V][H][W] (pt_denoise_views, the preview of a view frame), runs the
// plain or the kMasked kernels in their kViews form: the view is blockIdx.z, and every array is moved to that view's first pixel before
// anything is read.  From there on the kernel is the single frame's, bounds tests included, so no tap crosses a view border and view v is
// bit for bit what the single-frame run gives on view v alone.  kViews is a template parameter: the single-frame instantiations are untouched.
//
// pt_denoise_measured_run, the preview of a frame with its own measured variance (pt_denoise_measured, pt_frame_preview_measured; DESIGN.md
// 4.16; tests/denoise_measured_ref.py), runs the plain or the kMasked stages in their kMeasured form: a plane of (v_r, v_g, v_b, B) per pixel
// gives the variance of the mean of every pixel it rates (B >= 2), which replaces the 3x3 estimate there, and such a pixel filters with
// sigma_measured.  kMeasured is a parameter of the stage functions: the other kernels instantiate them without it, and with a plane
// that rates no pixel the kMeasured kernels compute what those do, operation for operation.
//
// One thread per pixel in 16 x 16 workgroups, float4 loads, fp32, no atomics: the result does not depend on the launch.  Every tap is
// read from global memory (L1/L2 serve the overlap of neighbouring workgroups); no tile is staged in LDS.
#include "pt_denoise.h"

#include <algorithm>

namespace {

#define PTDN_COVERED 1u
#define PTDN_EMISSIVE 2u
#define PTDN_HOLE 4u // kMasked only

constexpr float kAlbedoMin = 0.01f;
constexpr float kDepthRel = 1e-3f; // floor of the depth scale, relative to the pixel's own hit distance
constexpr float kLumEps = 1e-10f;
constexpr float kMinHistoryWeight = 1e-3f; // below this bilinear weight of valid taps a pixel has no history

// What the temporal form (pt_temporal_run) adds to the variance and a-trous kernels; unused (null) in pt_denoise's instantiation.
struct PtTemporalPixel {
    const int32_t *len;     // history length n of every pixel
    const float2 *moments;  // integrated luminance moments mu1, mu2
    int32_t min_history;    // moments_min_history
    float sigma_luminance_temporal;
};

// the pixel's variance comes from its temporal moments: a history of moments_min_history pushes and more (and never a pixel without history,
// so that a push without history is pt_denoise exactly)
__device__ __forceinline__ bool temporal_variance_px(const PtTemporalPixel &tp, int p) {
    const int32_t n = tp.len[p];
    return n >= tp.min_history && n >= 2;
}

// What the measured form (pt_denoise_measured_run) adds to the variance and a-trous stages; unused (null) in every other instantiation.
struct PtMeasuredPixel {
    const float4 *plane;   // per pixel (v_r, v_g, v_b, B): the measured variance of the pixel's mean and its batch means (pt_frame_get_variance)
    const float4 *feat;    // the frame's features: the albedo prepare divided by
    float sigma_measured;  // the luminance sigma of a rated pixel
};

// the pixel's variance is the measured one: two batch means and more, every v_c finite and not negative (false for NaN)
__device__ __forceinline__ bool measured_variance_px(float4 m) {
    const float top = 3.402823466e+38f;
    return m.w >= 2.0f && m.x >= 0.0f && m.x <= top && m.y >= 0.0f && m.y <= top && m.z >= 0.0f && m.z <= top;
}

// kViews: the first pixel of the workgroup's view in the stacked arrays
__device__ __forceinline__ size_t view_first_pixel(int32_t width, int32_t height) {
    return (size_t)blockIdx.z * ((size_t)width * (size_t)height);
}

__device__ __forceinline__ float lum_of(float r, float g, float b) {
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}

__device__ __forceinline__ float b3_tap(int k) { // k = -2 .. 2
    const int a = k < 0 ? -k : k;
    return a == 0 ? 3.0f / 8.0f : (a == 1 ? 1.0f / 4.0f : 1.0f / 16.0f);
}

__device__ __forceinline__ float normal_weight(float4 gp, float4 gq, float sigma_normal) {
    const float d = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
    return powf(fmaxf(0.0f, d), sigma_normal);
}

// |t_p - t_q| over the depth change the gradient predicts for the offset, floored relative to t_p (0 when the term is off, and 0 for
// equal distances whatever the scale: at t_p = 0 on a flat gradient the scale is 0, and 0 / 0 would make every weight NaN)
__device__ __forceinline__ float depth_arg(float tp, float tq, float2 g, float ox, float oy, float sigma_depth) {
    if(sigma_depth == 0.0f) {
        return 0.0f;
    }
    const float scale = sigma_depth * (fabsf(g.x * ox + g.y * oy) + kDepthRel * tp);
    const float d = fabsf(tp - tq);
    return d == 0.0f ? 0.0f : d / scale;
}

// kMasked: `samples` (the preview's sample counts) marks the holes, 0; a hole's colour is 0 whatever the input holds.
template<bool kMasked, bool kViews = false>
__global__ __launch_bounds__(256) void pt_denoise_prepare_kernel(const float4 *__restrict__ rgba, const float4 *__restrict__ feat, int32_t width, int32_t height,
                                                                 const int32_t *__restrict__ samples, float4 *__restrict__ col, float4 *__restrict__ guide,
                                                                 uint32_t *__restrict__ cls) {
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if(x >= width || y >= height) {
        return;
    }
    if constexpr(kViews) {
        const size_t v0 = view_first_pixel(width, height);
        rgba += v0;
        feat += 3 * v0;
        col += v0;
        guide += v0;
        cls += v0;
        if constexpr(kMasked) {
            samples += v0;
        }
    }
    const int p = y * width + x;
    const float4 f0 = feat[3 * p], f1 = feat[3 * p + 1], f2 = feat[3 * p + 2];
    const float4 c = rgba[p];
    const bool covered = f0.w > 0.0f, emissive = f2.w > 0.0f;
    float r = c.x, g = c.y, b = c.z;
    if(covered && !emissive) {
        r = r / fmaxf(f0.x, kAlbedoMin);
        g = g / fmaxf(f0.y, kAlbedoMin);
        b = b / fmaxf(f0.z, kAlbedoMin);
    }
    guide[p] = f1;
    if constexpr(kMasked) {
        if(samples[p] == 0) {
            col[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            cls[p] = (covered ? PTDN_COVERED : 0u) | (emissive ? PTDN_EMISSIVE : 0u) | PTDN_HOLE;
            return;
        }
    }
    col[p] = make_float4(r, g, b, lum_of(r, g, b));
    cls[p] = (covered ? PTDN_COVERED : 0u) | (emissive ? PTDN_EMISSIVE : 0u);
}

// kTemporal (pt_temporal_run): where the pixel's history is long enough (temporal_variance_px), its variance is that of the integrated
// luminance moments instead; the spatial estimate is computed as in pt_denoise either way.
// kMasked: a hole's variance is 0 (not filled yet); its gradient is computed as any pixel's (over neighbours of its class: holes).
// kMeasured (pt_denoise_measured_run): where the plane rates the pixel (measured_variance_px), its variance is the measured one instead:
// the standard deviation of every channel's mean in the unit of c (over the albedo floor prepare divided by, on the pixels it divided),
// their luminance -- the channels taken as fully correlated, DESIGN.md 4.16 -- squared.  The spatial estimate is computed either way.
template<bool kTemporal, bool kMasked, bool kViews, bool kMeasured>
__device__ __forceinline__ void denoise_variance_stage(const float4 *__restrict__ col, const float4 *__restrict__ guide, const uint32_t *__restrict__ cls,
                                                       int32_t width, int32_t height, float sigma_normal, float sigma_depth, float2 *__restrict__ grad,
                                                       float *__restrict__ var, const PtTemporalPixel &tp, const PtMeasuredPixel &mp) {
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if(x >= width || y >= height) {
        return;
    }
    if constexpr(kViews) {
        const size_t v0 = view_first_pixel(width, height);
        static_assert(!(kViews && kTemporal), "a view batch has no temporal form");
        col += v0;
        guide += v0;
        cls += v0;
        grad += v0;
        var += v0;
    }
    const int p = y * width + x;
    const uint32_t cp = cls[p];
    const float4 gp = guide[p];
    // gradient of t: central differences over neighbours of the same class, one-sided where only one is
    float2 gr = make_float2(0.0f, 0.0f);
    if(cp & PTDN_COVERED) {
        float d[2];
        for(int axis = 0; axis < 2; axis++) {
            const int dx = axis == 0 ? 1 : 0, dy = axis == 0 ? 0 : 1;
            const int xn = x + dx, yn = y + dy, xp = x - dx, yp = y - dy;
            const bool nxt = xn < width && yn < height && cls[yn * width + xn] == cp;
            const bool prv = xp >= 0 && yp >= 0 && cls[yp * width + xp] == cp;
            const float tn = nxt ? guide[yn * width + xn].w : 0.0f, tq = prv ? guide[yp * width + xp].w : 0.0f;
            d[axis] = (nxt && prv) ? (tn - tq) * 0.5f : (nxt ? tn - gp.w : (prv ? gp.w - tq : 0.0f));
        }
        gr = make_float2(d[0], d[1]);
    }
    grad[p] = gr;
    if constexpr(kMasked) {
        if(cp & PTDN_HOLE) {
            var[p] = 0.0f;
            return;
        }
    }
    float sw = 0.0f, m1 = 0.0f, m2 = 0.0f;
    for(int dy = -1; dy <= 1; dy++) {
        for(int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if(qx < 0 || qy < 0 || qx >= width || qy >= height) {
                continue;
            }
            const int q = qy * width + qx;
            const float lq = col[q].w;
            float w;
            if(dx == 0 && dy == 0) {
                w = 1.0f;
            }
            else if((cp & PTDN_COVERED) && cls[q] == cp) {
                const float4 gq = guide[q];
                w = normal_weight(gp, gq, sigma_normal) * expf(-depth_arg(gp.w, gq.w, gr, (float)dx, (float)dy, sigma_depth));
            }
            else {
                continue; // (a zero weight: adds nothing, whatever the tap holds)
            }
            sw = sw + w;
            m1 = m1 + w * lq;
            m2 = m2 + w * (lq * lq);
        }
    }
    const float mean = m1 / sw;
    float v = fmaxf(0.0f, m2 / sw - mean * mean);
    if constexpr(kTemporal) {
        if(temporal_variance_px(tp, p)) {
            const float2 m = tp.moments[p];
            v = fmaxf(0.0f, m.y - m.x * m.x);
        }
    }
    if constexpr(kMeasured) {
        const float4 m = mp.plane[p];
        if(measured_variance_px(m)) {
            float sr = sqrtf(m.x), sg = sqrtf(m.y), sb = sqrtf(m.z);
            if((cp & PTDN_COVERED) && !(cp & PTDN_EMISSIVE)) {
                const float4 f0 = mp.feat[3 * p];
                sr = sr / fmaxf(f0.x, kAlbedoMin);
                sg = sg / fmaxf(f0.y, kAlbedoMin);
                sb = sb / fmaxf(f0.z, kAlbedoMin);
            }
            const float s = lum_of(sr, sg, sb);
            v = s * s;
        }
    }
    var[p] = v;
}

template<bool kTemporal, bool kMasked, bool kViews = false>
__global__ __launch_bounds__(256) void pt_denoise_variance_kernel(const float4 *__restrict__ col, const float4 *__restrict__ guide, const uint32_t *__restrict__ cls,
                                                                  int32_t width, int32_t height, float sigma_normal, float sigma_depth, float2 *__restrict__ grad,
                                                                  float *__restrict__ var, PtTemporalPixel tp) {
    denoise_variance_stage<kTemporal, kMasked, kViews, false>(col, guide, cls, width, height, sigma_normal, sigma_depth, grad, var, tp, PtMeasuredPixel{});
}

template<bool kMasked>
__global__ __launch_bounds__(256) void pt_denoise_variance_measured_kernel(const float4 *__restrict__ col, const float4 *__restrict__ guide,
                                                                           const uint32_t *__restrict__ cls, int32_t width, int32_t height, float sigma_normal,
                                                                           float sigma_depth, float2 *__restrict__ grad, float *__restrict__ var, PtMeasuredPixel mp) {
    denoise_variance_stage<false, kMasked, false, true>(col, guide, cls, width, height, sigma_normal, sigma_depth, grad, var, PtTemporalPixel{}, mp);
}

// kTemporal: the luminance sigma is tp.sigma_luminance_temporal at pixels whose variance came from the temporal moments.
// kMasked: holes are no taps (the variance prefilter included), and a hole is filled (pt_denoise_masked_run).
// kMeasured: the luminance sigma is mp.sigma_measured at pixels whose variance is the measured one.
template<bool kTemporal, bool kMasked, bool kViews, bool kMeasured>
__device__ __forceinline__ void denoise_atrous_stage(const float4 *__restrict__ col_in, const float *__restrict__ var_in, const float4 *__restrict__ guide,
                                                     const uint32_t *__restrict__ cls, const float2 *__restrict__ grad, int32_t width, int32_t height,
                                                     int32_t step, float sigma_luminance, float sigma_normal, float sigma_depth,
                                                     float4 *__restrict__ col_out, float *__restrict__ var_out, const PtTemporalPixel &tp,
                                                     const PtMeasuredPixel &mp) {
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if(x >= width || y >= height) {
        return;
    }
    if constexpr(kViews) {
        const size_t v0 = view_first_pixel(width, height);
        static_assert(!(kViews && kTemporal), "a view batch has no temporal form");
        col_in += v0;
        var_in += v0;
        guide += v0;
        cls += v0;
        grad += v0;
        col_out += v0;
        var_out += v0;
    }
    const int p = y * width + x;
    const uint32_t cp = cls[p];
    if constexpr(kMasked) {
        if(cp & PTDN_HOLE) {
            const uint32_t want = cp & ~PTDN_HOLE; // taps of the hole's class that are not holes
            const float4 gp = guide[p];
            const float2 gr = grad[p];
            float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
            for(int dy = -2; dy <= 2; dy++) {
                for(int dx = -2; dx <= 2; dx++) {
                    const int ox = dx * step, oy = dy * step;
                    const int qx = x + ox, qy = y + oy;
                    if((dx == 0 && dy == 0) || qx < 0 || qy < 0 || qx >= width || qy >= height) {
                        continue;
                    }
                    const int q = qy * width + qx;
                    if(cls[q] != want) {
                        continue;
                    }
                    const float h = b3_tap(dy) * b3_tap(dx);
                    float w = h;
                    if(cp & PTDN_COVERED) {
                        const float4 gq = guide[q];
                        w = (h * normal_weight(gp, gq, sigma_normal)) * expf(-depth_arg(gp.w, gq.w, gr, (float)ox, (float)oy, sigma_depth));
                    }
                    const float4 cq = col_in[q];
                    sw = sw + w;
                    sr = sr + w * cq.x;
                    sg = sg + w * cq.y;
                    sb = sb + w * cq.z;
                }
            }
            if(sw > 0.0f) {
                const float r = sr / sw, gg = sg / sw, b = sb / sw;
                col_out[p] = make_float4(r, gg, b, lum_of(r, gg, b));
                var_out[p] = 1.0f;
            }
            else {
                col_out[p] = col_in[p];
                var_out[p] = var_in[p];
            }
            return;
        }
    }
    if(!(cp & PTDN_COVERED)) { // no ray hit: nothing to filter against
        col_out[p] = col_in[p];
        var_out[p] = var_in[p];
        return;
    }
    // the variance behind the luminance weight, prefiltered with a 3x3 binomial kernel (taps inside the image)
    float g = 0.0f, gs = 0.0f;
    for(int dy = -1; dy <= 1; dy++) {
        for(int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if(qx < 0 || qy < 0 || qx >= width || qy >= height) {
                continue;
            }
            if constexpr(kMasked) {
                if(cls[qy * width + qx] & PTDN_HOLE) {
                    continue;
                }
            }
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            g = g + k * var_in[qy * width + qx];
            gs = gs + k;
        }
    }
    g = g / gs;
    float sl = sigma_luminance;
    if constexpr(kTemporal) {
        if(temporal_variance_px(tp, p)) {
            sl = tp.sigma_luminance_temporal;
        }
    }
    if constexpr(kMeasured) {
        if(measured_variance_px(mp.plane[p])) {
            sl = mp.sigma_measured;
        }
    }
    const float lum_scale = sl * sqrtf(g) + kLumEps;
    const float4 gp = guide[p];
    const float2 gr = grad[p];
    const float lp = col_in[p].w;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    for(int dy = -2; dy <= 2; dy++) {
        for(int dx = -2; dx <= 2; dx++) {
            const int ox = dx * step, oy = dy * step;
            const int qx = x + ox, qy = y + oy;
            if(qx < 0 || qy < 0 || qx >= width || qy >= height) {
                continue;
            }
            const int q = qy * width + qx;
            const float h = b3_tap(dy) * b3_tap(dx);
            float w;
            if(dx == 0 && dy == 0) {
                w = h;
            }
            else if(cls[q] == cp) {
                const float4 gq = guide[q];
                float a = depth_arg(gp.w, gq.w, gr, (float)ox, (float)oy, sigma_depth);
                if(sl != 0.0f) {
                    a = a + fabsf(lp - col_in[q].w) / lum_scale;
                }
                w = (h * normal_weight(gp, gq, sigma_normal)) * expf(-a);
            }
            else {
                continue; // (a zero weight: adds nothing)
            }
            const float4 cq = col_in[q];
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
            sv = sv + (w * w) * var_in[q];
        }
    }
    const float r = sr / sw, gg = sg / sw, b = sb / sw;
    col_out[p] = make_float4(r, gg, b, lum_of(r, gg, b));
    var_out[p] = sv / (sw * sw);
}

template<bool kTemporal, bool kMasked, bool kViews = false>
__global__ __launch_bounds__(256) void pt_denoise_atrous_kernel(const float4 *__restrict__ col_in, const float *__restrict__ var_in, const float4 *__restrict__ guide,
                                                                const uint32_t *__restrict__ cls, const float2 *__restrict__ grad, int32_t width, int32_t height,
                                                                int32_t step, float sigma_luminance, float sigma_normal, float sigma_depth,
                                                                float4 *__restrict__ col_out, float *__restrict__ var_out, PtTemporalPixel tp) {
    denoise_atrous_stage<kTemporal, kMasked, kViews, false>(col_in, var_in, guide, cls, grad, width, height, step, sigma_luminance, sigma_normal, sigma_depth, col_out,
                                                            var_out, tp, PtMeasuredPixel{});
}

template<bool kMasked>
__global__ __launch_bounds__(256) void pt_denoise_atrous_measured_kernel(const float4 *__restrict__ col_in, const float *__restrict__ var_in,
                                                                         const float4 *__restrict__ guide, const uint32_t *__restrict__ cls,
                                                                         const float2 *__restrict__ grad, int32_t width, int32_t height, int32_t step,
                                                                         float sigma_luminance, float sigma_normal, float sigma_depth, float4 *__restrict__ col_out,
                                                                         float *__restrict__ var_out, PtMeasuredPixel mp) {
    denoise_atrous_stage<false, kMasked, false, true>(col_in, var_in, guide, cls, grad, width, height, step, sigma_luminance, sigma_normal, sigma_depth, col_out,
                                                      var_out, PtTemporalPixel{}, mp);
}

// the previous push's history, as the temporal step reads it
struct PtTemporalPrev {
    const float4 *col;
    const float2 *moments;
    const int32_t *len;
    const float4 *pos, *nrm;
    const uint32_t *cls;
};

struct PtTemporalBlend {
    float alpha_color, alpha_moments;
    int32_t max_history;
    float normal_min, position_tolerance;
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// Temporal step of pt_temporal_run: reprojects every covered pixel's first-hit position into the previous push's camera, gathers the
// previous push's history at the 2x2 bilinear taps that see the same surface, and blends.  Only + - * /, one square root and comparisons,
// all correctly rounded (the build has -ffp-contract=off), so the history lengths equal tests/temporal_ref.py's exactly.
//
// kMotion (pt_temporal_run_motion; include/pt_motion.h): `motion` says where the pixel's surface was at the previous pose.
// A pixel with rays that had no previous position (motion[1].w > 0) has no history.  Otherwise Xr = motion[0].xyz / coverage and nr =
// motion[1].xyz at unit length are what is reprojected and what the taps' normal and position tests compare; the pixel is its own tap
// only under the same camera AND with no ray on a moved surface (motion[0].w == 0), every other pixel projects Xr into the previous
// camera (rp's origin and rows are filled whenever there is a previous push).  The tolerance's t and what is stored for the next push
// stay the current frame's.  The plain kernel is the kMotion = false instantiation: `motion` is not read.
template<bool kMotion>
__device__ __forceinline__ void temporal_accumulate(const float4 *__restrict__ feat, const float4 *__restrict__ col_in, const uint32_t *__restrict__ cls, int32_t width,
                                                    int32_t height, const PtReprojection &rp, const PtTemporalPrev &prev, const PtTemporalBlend &bl,
                                                    float4 *__restrict__ col_out, float2 *__restrict__ mom_out, int32_t *__restrict__ len_out,
                                                    float4 *__restrict__ pos_out, float4 *__restrict__ nrm_out, const float4 *__restrict__ motion) {
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if(x >= width || y >= height) {
        return;
    }
    const int p = y * width + x;
    const float4 c = col_in[p];
    const float l = c.w;
    const uint32_t cp = cls[p];
    if(!(cp & PTDN_COVERED)) { // no ray hit: the input stays, no history
        col_out[p] = c;
        mom_out[p] = make_float2(l, l * l);
        len_out[p] = 0;
        pos_out[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        nrm_out[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 f0 = feat[3 * p], f1 = feat[3 * p + 1], f2 = feat[3 * p + 2];
    const float cov = f0.w;
    const float X = f2.x / cov, Y = f2.y / cov, Z = f2.z / cov;          // mean hit position of the rays that hit
    const float t = f1.w / cov;                                          // ... and hit distance
    const float len2 = dot3(f1.x, f1.y, f1.z, f1.x, f1.y, f1.z);         // their mean normal at unit length (a pixel on an edge matches itself)
    const float inv = 1.0f / sqrtf(len2);
    const float nx = len2 > 0.0f ? f1.x * inv : 0.0f, ny = len2 > 0.0f ? f1.y * inv : 0.0f, nz = len2 > 0.0f ? f1.z * inv : 0.0f;
    pos_out[p] = make_float4(X, Y, Z, 0.0f);
    nrm_out[p] = make_float4(nx, ny, nz, 0.0f);

    // what is reprojected and compared with the taps: the pixel's own position and normal, or (kMotion) those it had at the previous pose
    float Xr = X, Yr = Y, Zr = Z, nrx = nx, nry = ny, nrz = nz;
    bool own_tap = rp.mode == PT_REPROJECT_IDENTICAL, project = rp.mode == PT_REPROJECT_CAMERA;
    if constexpr(kMotion) {
        const float4 m0 = motion[2 * p], m1 = motion[2 * p + 1];
        Xr = m0.x / cov;
        Yr = m0.y / cov;
        Zr = m0.z / cov;
        const float mlen2 = dot3(m1.x, m1.y, m1.z, m1.x, m1.y, m1.z);
        const float minv = 1.0f / sqrtf(mlen2);
        nrx = mlen2 > 0.0f ? m1.x * minv : 0.0f;
        nry = mlen2 > 0.0f ? m1.y * minv : 0.0f;
        nrz = mlen2 > 0.0f ? m1.z * minv : 0.0f;
        const bool had_position = !(m1.w > 0.0f);
        project = had_position && (project || (own_tap && !(m0.w == 0.0f)));
        own_tap = had_position && own_tap && m0.w == 0.0f;
    }
    float px = 0.0f, py = 0.0f;
    bool found = false;
    if(own_tap) {
        px = (float)x;
        py = (float)y;
        found = true;
    }
    else if(project) {
        // X - origin = a forward + b up + c right; the rows are the inverse of [forward up right] times |det|
        const float dx = Xr - rp.origin[0], dy = Yr - rp.origin[1], dz = Zr - rp.origin[2];
        const float a = dot3(dx, dy, dz, rp.row[0][0], rp.row[0][1], rp.row[0][2]);
        const float b = dot3(dx, dy, dz, rp.row[1][0], rp.row[1][1], rp.row[1][2]);
        const float cc = dot3(dx, dy, dz, rp.row[2][0], rp.row[2][1], rp.row[2][2]);
        if(a > 0.0f) { // in front of the previous camera
            const float xc = cc / a, yc = b / a;
            // worker.cpp: x_camera = 2 ((x + 1/2) / W - 1/2), y_camera = -2 ((y + 1/2) / H - 1/2)
            px = (xc * 0.5f + 0.5f) * (float)width - 0.5f;
            py = (0.5f - yc * 0.5f) * (float)height - 0.5f;
            found = px > -2.0f && px < (float)width + 1.0f && py > -2.0f && py < (float)height + 1.0f; // (false for NaN)
        }
    }
    int32_t n = 1;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, s1 = 0.0f, s2 = 0.0f;
    if(found) {
        const int x0 = (int)floorf(px), y0 = (int)floorf(py);
        const float fx = px - (float)x0, fy = py - (float)y0;
        const float r = bl.position_tolerance * (t * rp.footprint);
        const float r2 = r * r;
        int32_t nmax = 0;
        for(int k = 0; k < 4; k++) {
            const int ox = k & 1, oy = k >> 1;
            const float w = (ox ? fx : 1.0f - fx) * (oy ? fy : 1.0f - fy);
            const int qx = x0 + ox, qy = y0 + oy;
            if(!(w > 0.0f) || qx < 0 || qy < 0 || qx >= width || qy >= height) {
                continue;
            }
            const int q = qy * width + qx;
            if(prev.cls[q] != cp) {
                continue;
            }
            const float4 nq = prev.nrm[q];
            if(!(dot3(nrx, nry, nrz, nq.x, nq.y, nq.z) >= bl.normal_min)) {
                continue;
            }
            const float4 xq = prev.pos[q];
            const float ex = Xr - xq.x, ey = Yr - xq.y, ez = Zr - xq.z;
            if(!(dot3(ex, ey, ez, ex, ey, ez) <= r2)) {
                continue;
            }
            const float4 hc = prev.col[q];
            const float2 hm = prev.moments[q];
            sw = sw + w;
            sr = sr + w * hc.x;
            sg = sg + w * hc.y;
            sb = sb + w * hc.z;
            s1 = s1 + w * hm.x;
            s2 = s2 + w * hm.y;
            nmax = max(nmax, prev.len[q]);
        }
        if(!(sw < kMinHistoryWeight)) {
            n = min(1 + nmax, bl.max_history);
        }
    }
    len_out[p] = n;
    if(n == 1) { // no history: the current frame as it is
        col_out[p] = c;
        mom_out[p] = make_float2(l, l * l);
        return;
    }
    const float inv_n = 1.0f / (float)n;
    const float ac = fmaxf(inv_n, bl.alpha_color), am = fmaxf(inv_n, bl.alpha_moments);
    const float r = (1.0f - ac) * (sr / sw) + ac * c.x;
    const float g = (1.0f - ac) * (sg / sw) + ac * c.y;
    const float b = (1.0f - ac) * (sb / sw) + ac * c.z;
    col_out[p] = make_float4(r, g, b, lum_of(r, g, b));
    mom_out[p] = make_float2((1.0f - am) * (s1 / sw) + am * l, (1.0f - am) * (s2 / sw) + am * (l * l));
}

__global__ __launch_bounds__(256) void pt_temporal_accumulate_kernel(const float4 *__restrict__ feat, const float4 *__restrict__ col_in,
                                                                     const uint32_t *__restrict__ cls, int32_t width, int32_t height, PtReprojection rp,
                                                                     PtTemporalPrev prev, PtTemporalBlend bl, float4 *__restrict__ col_out,
                                                                     float2 *__restrict__ mom_out, int32_t *__restrict__ len_out, float4 *__restrict__ pos_out,
                                                                     float4 *__restrict__ nrm_out) {
    temporal_accumulate<false>(feat, col_in, cls, width, height, rp, prev, bl, col_out, mom_out, len_out, pos_out, nrm_out, nullptr);
}

__global__ __launch_bounds__(256) void pt_temporal_accumulate_motion_kernel(const float4 *__restrict__ feat, const float4 *__restrict__ col_in,
                                                                            const uint32_t *__restrict__ cls, int32_t width, int32_t height, PtReprojection rp,
                                                                            PtTemporalPrev prev, PtTemporalBlend bl, float4 *__restrict__ col_out,
                                                                            float2 *__restrict__ mom_out, int32_t *__restrict__ len_out,
                                                                            float4 *__restrict__ pos_out, float4 *__restrict__ nrm_out,
                                                                            const float4 *__restrict__ motion) {
    temporal_accumulate<true>(feat, col_in, cls, width, height, rp, prev, bl, col_out, mom_out, len_out, pos_out, nrm_out, motion);
}

// (rgba and out may be the same array: no __restrict__ on them)
// kMasked: a hole that a pass filled has alpha 1, one that none did is (0, 0, 0, 0).
template<bool kMasked, bool kViews = false>
__global__ __launch_bounds__(256) void pt_denoise_finish_kernel(const float4 *__restrict__ col, const float4 *rgba, const float4 *__restrict__ feat, int32_t width,
                                                                int32_t height, const uint32_t *__restrict__ cls, const float *__restrict__ var, float4 *out) {
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if(x >= width || y >= height) {
        return;
    }
    if constexpr(kViews) {
        const size_t v0 = view_first_pixel(width, height);
        col += v0;
        rgba += v0;
        feat += 3 * v0;
        out += v0;
        if constexpr(kMasked) {
            cls += v0;
            var += v0;
        }
    }
    const int p = y * width + x;
    const float4 f0 = feat[3 * p], f2 = feat[3 * p + 2];
    const float4 c = col[p];
    float alpha = rgba[p].w;
    if constexpr(kMasked) {
        if(cls[p] & PTDN_HOLE) {
            if(!(var[p] > 0.0f)) {
                out[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                return;
            }
            alpha = 1.0f;
        }
    }
    float4 o = make_float4(c.x, c.y, c.z, alpha);
    if(f0.w > 0.0f && !(f2.w > 0.0f)) {
        o.x = c.x * fmaxf(f0.x, kAlbedoMin);
        o.y = c.y * fmaxf(f0.y, kAlbedoMin);
        o.z = c.z * fmaxf(f0.z, kAlbedoMin);
    }
    out[p] = o;
}

} // namespace

hipError_t pt_denoise_run(hipStream_t stream, const float4 *rgba, const float4 *features, int32_t width, int32_t height, const PtDenoiseParams &params,
                          const PtDenoiseScratch &s, float4 *out) {
    const dim3 block(16, 16), grid((width + 15) / 16, (height + 15) / 16);
    hipLaunchKernelGGL(pt_denoise_prepare_kernel<false>, grid, block, 0, stream, rgba, features, width, height, nullptr, s.col[0], s.guide, s.cls);
    hipLaunchKernelGGL((pt_denoise_variance_kernel<false, false>), grid, block, 0, stream, s.col[0], s.guide, s.cls, width, height, params.sigma_normal,
                       params.sigma_depth, s.grad, s.var[0], PtTemporalPixel{});
    int cur = 0;
    for(int i = 0; i < params.iterations; i++) {
        hipLaunchKernelGGL((pt_denoise_atrous_kernel<false, false>), grid, block, 0, stream, s.col[cur], s.var[cur], s.guide, s.cls, s.grad, width, height, 1 << i,
                           params.sigma_luminance, params.sigma_normal, params.sigma_depth, s.col[cur ^ 1], s.var[cur ^ 1], PtTemporalPixel{});
        cur ^= 1;
    }
    hipLaunchKernelGGL(pt_denoise_finish_kernel<false>, grid, block, 0, stream, s.col[cur], rgba, features, width, height, nullptr, nullptr, out);
    return hipGetLastError();
}

hipError_t pt_denoise_masked_run(hipStream_t stream, const float4 *rgba, const float4 *features, const int32_t *samples, int32_t width, int32_t height,
                                 const PtDenoiseParams &params, const PtDenoiseScratch &s, float4 *out) {
    const dim3 block(16, 16), grid((width + 15) / 16, (height + 15) / 16);
    hipLaunchKernelGGL(pt_denoise_prepare_kernel<true>, grid, block, 0, stream, rgba, features, width, height, samples, s.col[0], s.guide, s.cls);
    hipLaunchKernelGGL((pt_denoise_variance_kernel<false, true>), grid, block, 0, stream, s.col[0], s.guide, s.cls, width, height, params.sigma_normal,
                       params.sigma_depth, s.grad, s.var[0], PtTemporalPixel{});
    int cur = 0;
    for(int i = 0; i < params.iterations; i++) {
        hipLaunchKernelGGL((pt_denoise_atrous_kernel<false, true>), grid, block, 0, stream, s.col[cur], s.var[cur], s.guide, s.cls, s.grad, width, height, 1 << i,
                           params.sigma_luminance, params.sigma_normal, params.sigma_depth, s.col[cur ^ 1], s.var[cur ^ 1], PtTemporalPixel{});
        cur ^= 1;
    }
    hipLaunchKernelGGL(pt_denoise_finish_kernel<true>, grid, block, 0, stream, s.col[cur], rgba, features, width, height, s.cls, s.var[cur], out);
    return hipGetLastError();
}

namespace {

template<bool kMasked>
hipError_t run_measured(hipStream_t stream, const float4 *rgba, const float4 *features, const float4 *variance, const int32_t *samples, int32_t width, int32_t height,
                        const PtDenoiseParams &params, float sigma_measured, const PtDenoiseScratch &s, float4 *out) {
    const dim3 block(16, 16), grid((width + 15) / 16, (height + 15) / 16);
    const PtMeasuredPixel mp{variance, features, sigma_measured};
    hipLaunchKernelGGL(pt_denoise_prepare_kernel<kMasked>, grid, block, 0, stream, rgba, features, width, height, samples, s.col[0], s.guide, s.cls);
    hipLaunchKernelGGL(pt_denoise_variance_measured_kernel<kMasked>, grid, block, 0, stream, s.col[0], s.guide, s.cls, width, height, params.sigma_normal,
                       params.sigma_depth, s.grad, s.var[0], mp);
    int cur = 0;
    for(int i = 0; i < params.iterations; i++) {
        hipLaunchKernelGGL(pt_denoise_atrous_measured_kernel<kMasked>, grid, block, 0, stream, s.col[cur], s.var[cur], s.guide, s.cls, s.grad, width, height, 1 << i,
                           params.sigma_luminance, params.sigma_normal, params.sigma_depth, s.col[cur ^ 1], s.var[cur ^ 1], mp);
        cur ^= 1;
    }
    hipLaunchKernelGGL(pt_denoise_finish_kernel<kMasked>, grid, block, 0, stream, s.col[cur], rgba, features, width, height, kMasked ? s.cls : nullptr,
                       kMasked ? s.var[cur] : nullptr, out);
    return hipGetLastError();
}

} // namespace

hipError_t pt_denoise_measured_run(hipStream_t stream, const float4 *rgba, const float4 *features, const float4 *variance, const int32_t *samples, int32_t width,
                                   int32_t height, const PtDenoiseParams &params, float sigma_measured, const PtDenoiseScratch &scratch, float4 *out) {
    return samples != nullptr ? run_measured<true>(stream, rgba, features, variance, samples, width, height, params, sigma_measured, scratch, out)
                              : run_measured<false>(stream, rgba, features, variance, nullptr, width, height, params, sigma_measured, scratch, out);
}

namespace {

// The kViews launches of `count` views from view `first` on: 3 + iterations launches, the view in blockIdx.z
template<bool kMasked>
hipError_t run_views(hipStream_t stream, const float4 *rgba, const float4 *features, const int32_t *samples, int32_t width, int32_t height, size_t first,
                     uint32_t count, const PtDenoiseParams &params, const PtDenoiseScratch &scratch, float4 *out) {
    const size_t at = first * (static_cast<size_t>(width) * static_cast<size_t>(height));
    rgba += at;
    features += 3 * at;
    out += at;
    if(samples != nullptr) {
        samples += at;
    }
    PtDenoiseScratch s = scratch;
    s.col[0] += at;
    s.col[1] += at;
    s.var[0] += at;
    s.var[1] += at;
    s.guide += at;
    s.grad += at;
    s.cls += at;
    const dim3 block(16, 16), grid((width + 15) / 16, (height + 15) / 16, count);
    hipLaunchKernelGGL((pt_denoise_prepare_kernel<kMasked, true>), grid, block, 0, stream, rgba, features, width, height, samples, s.col[0], s.guide, s.cls);
    hipLaunchKernelGGL((pt_denoise_variance_kernel<false, kMasked, true>), grid, block, 0, stream, s.col[0], s.guide, s.cls, width, height, params.sigma_normal,
                       params.sigma_depth, s.grad, s.var[0], PtTemporalPixel{});
    int cur = 0;
    for(int i = 0; i < params.iterations; i++) {
        hipLaunchKernelGGL((pt_denoise_atrous_kernel<false, kMasked, true>), grid, block, 0, stream, s.col[cur], s.var[cur], s.guide, s.cls, s.grad, width, height,
                           1 << i, params.sigma_luminance, params.sigma_normal, params.sigma_depth, s.col[cur ^ 1], s.var[cur ^ 1], PtTemporalPixel{});
        cur ^= 1;
    }
    hipLaunchKernelGGL((pt_denoise_finish_kernel<kMasked, true>), grid, block, 0, stream, s.col[cur], rgba, features, width, height, kMasked ? s.cls : nullptr,
                       kMasked ? s.var[cur] : nullptr, out);
    return hipGetLastError();
}

} // namespace

hipError_t pt_denoise_views_run(hipStream_t stream, const float4 *rgba, const float4 *features, const int32_t *samples, int32_t width, int32_t height,
                                int32_t n_views, const PtDenoiseParams &params, const PtDenoiseScratch &scratch, float4 *out) {
    if(n_views == 1) { // the single frame's own launches
        return samples != nullptr ? pt_denoise_masked_run(stream, rgba, features, samples, width, height, params, scratch, out)
                                  : pt_denoise_run(stream, rgba, features, width, height, params, scratch, out);
    }
    // (a grid has 65535 planes at most: a longer batch takes one set of launches per 65535 views, each on its own part of every array)
    constexpr size_t kMaxPlanes = 65535;
    for(size_t first = 0; first < static_cast<size_t>(n_views); first += kMaxPlanes) {
        const uint32_t count = static_cast<uint32_t>(std::min(kMaxPlanes, static_cast<size_t>(n_views) - first));
        const hipError_t e = samples != nullptr ? run_views<true>(stream, rgba, features, samples, width, height, first, count, params, scratch, out)
                                                : run_views<false>(stream, rgba, features, nullptr, width, height, first, count, params, scratch, out);
        if(e != hipSuccess) {
            return e;
        }
    }
    return hipSuccess;
}

namespace {

// pt_temporal_run (motion == nullptr) and pt_temporal_run_motion
hipError_t temporal_run(hipStream_t stream, const float4 *rgba, const float4 *features, const float4 *motion, int32_t width, int32_t height, const PtTemporalParams &params,
                        const PtReprojection &reprojection, const PtDenoiseScratch &scratch, const PtTemporalState &state, float4 *out) {
    const dim3 block(16, 16), grid((width + 15) / 16, (height + 15) / 16);
    const int cur = state.cur, prv = state.cur ^ 1;
    PtDenoiseScratch s = scratch;
    s.cls = state.cls[cur];
    // prepare -> col[1]; integrate -> col[0]; a-trous pass 0 -> the colour history; passes 1.. alternate col[1], col[0], ...
    hipLaunchKernelGGL(pt_denoise_prepare_kernel<false>, grid, block, 0, stream, rgba, features, width, height, nullptr, s.col[1], s.guide, s.cls);
    const PtTemporalPrev prev{state.col_hist, state.moments[prv], state.len[prv], state.pos[prv], state.nrm[prv], state.cls[prv]};
    const PtTemporalBlend bl{params.alpha_color, params.alpha_moments, params.max_history, params.normal_min, params.position_tolerance};
    if(motion != nullptr) {
        hipLaunchKernelGGL(pt_temporal_accumulate_motion_kernel, grid, block, 0, stream, features, s.col[1], s.cls, width, height, reprojection, prev, bl, s.col[0],
                           state.moments[cur], state.len[cur], state.pos[cur], state.nrm[cur], motion);
    }
    else {
        hipLaunchKernelGGL(pt_temporal_accumulate_kernel, grid, block, 0, stream, features, s.col[1], s.cls, width, height, reprojection, prev, bl, s.col[0],
                           state.moments[cur], state.len[cur], state.pos[cur], state.nrm[cur]);
    }
    const PtTemporalPixel tp{state.len[cur], state.moments[cur], params.moments_min_history, params.sigma_luminance_temporal};
    const PtDenoiseParams &sp = params.spatial;
    hipLaunchKernelGGL((pt_denoise_variance_kernel<true, false>), grid, block, 0, stream, s.col[0], s.guide, s.cls, width, height, sp.sigma_normal, sp.sigma_depth,
                       s.grad, s.var[0], tp);
    const float4 *col = s.col[0];
    int v = 0;
    for(int i = 0; i < sp.iterations; i++) {
        float4 *dst = i == 0 ? state.col_hist : s.col[i & 1];
        hipLaunchKernelGGL((pt_denoise_atrous_kernel<true, false>), grid, block, 0, stream, col, s.var[v], s.guide, s.cls, s.grad, width, height, 1 << i,
                           sp.sigma_luminance, sp.sigma_normal, sp.sigma_depth, dst, s.var[v ^ 1], tp);
        col = dst;
        v ^= 1;
    }
    if(sp.iterations == 0) { // the integrated colour is the history
        const hipError_t e = hipMemcpyAsync(state.col_hist, s.col[0], static_cast<size_t>(width) * height * sizeof(float4), hipMemcpyDeviceToDevice, stream);
        if(e != hipSuccess) {
            return e;
        }
    }
    hipLaunchKernelGGL(pt_denoise_finish_kernel<false>, grid, block, 0, stream, col, rgba, features, width, height, nullptr, nullptr, out);
    return hipGetLastError();
}

} // namespace

hipError_t pt_temporal_run(hipStream_t stream, const float4 *rgba, const float4 *features, int32_t width, int32_t height, const PtTemporalParams &params,
                           const PtReprojection &reprojection, const PtDenoiseScratch &scratch, const PtTemporalState &state, float4 *out) {
    return temporal_run(stream, rgba, features, nullptr, width, height, params, reprojection, scratch, state, out);
}

hipError_t pt_temporal_run_motion(hipStream_t stream, const float4 *rgba, const float4 *features, const float4 *motion, int32_t width, int32_t height,
                                  const PtTemporalParams &params, const PtReprojection &reprojection, const PtDenoiseScratch &scratch, const PtTemporalState &state,
                                  float4 *out) {
    return temporal_run(stream, rgba, features, motion, width, height, params, reprojection, scratch, state, out);
}
