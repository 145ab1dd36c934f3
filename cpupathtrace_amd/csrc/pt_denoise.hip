// pt_denoise.hip -- feature-guided denoising of a finished frame (RenderOptions::allow_bias): the spatial part of SVGF (Schied et al. 2017)
// on the features of pt_feature_kernel (pt_path.hip).  DESIGN.md 4.10 has the algorithm, its constants and its measured cost;
// tests/denoise_ref.py restates every kernel below in numpy, operation for operation.
//
//   prepare   c = rgb / max(albedo, 0.01) on covered, non-emissive pixels (rgb elsewhere), its luminance, the guide (n, t), the class
//   variance  the hit distance's screen-space gradient and the luminance variance over the edge-aware 3x3 neighbourhood
//   atrous    one pass of the 5x5 B3-spline kernel at step 2^i with normal, depth and luminance weights (variance: squared weights)
//   finish    rgb = c * the factor of `prepare`, alpha copied from the input
//
// One thread per pixel in 16 x 16 workgroups, float4 loads, fp32, no atomics: the result does not depend on the launch.  Every tap is
// read from global memory (L1/L2 serve the overlap of neighbouring workgroups); no tile is staged in LDS.
#include "pt_denoise.h"

namespace {

#define PTDN_COVERED 1u
#define PTDN_EMISSIVE 2u

constexpr float kAlbedoMin = 0.01f;
constexpr float kDepthRel = 1e-3f; // floor of the depth scale, relative to the pixel's own hit distance
constexpr float kLumEps = 1e-10f;

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

// |t_p - t_q| over the depth change the gradient predicts for the offset, floored relative to t_p (0 when the term is off)
__device__ __forceinline__ float depth_arg(float tp, float tq, float2 g, float ox, float oy, float sigma_depth) {
    if(sigma_depth == 0.0f) {
        return 0.0f;
    }
    const float scale = sigma_depth * (fabsf(g.x * ox + g.y * oy) + kDepthRel * tp);
    return fabsf(tp - tq) / scale;
}

__global__ __launch_bounds__(256) void pt_denoise_prepare_kernel(const float4 *__restrict__ rgba, const float4 *__restrict__ feat, int32_t width, int32_t height,
                                                                 float4 *__restrict__ col, float4 *__restrict__ guide, uint32_t *__restrict__ cls) {
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if(x >= width || y >= height) {
        return;
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
    col[p] = make_float4(r, g, b, lum_of(r, g, b));
    guide[p] = f1;
    cls[p] = (covered ? PTDN_COVERED : 0u) | (emissive ? PTDN_EMISSIVE : 0u);
}

__global__ __launch_bounds__(256) void pt_denoise_variance_kernel(const float4 *__restrict__ col, const float4 *__restrict__ guide, const uint32_t *__restrict__ cls,
                                                                  int32_t width, int32_t height, float sigma_normal, float sigma_depth, float2 *__restrict__ grad,
                                                                  float *__restrict__ var) {
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if(x >= width || y >= height) {
        return;
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
                w = 0.0f;
            }
            sw = sw + w;
            m1 = m1 + w * lq;
            m2 = m2 + w * (lq * lq);
        }
    }
    const float mean = m1 / sw;
    var[p] = fmaxf(0.0f, m2 / sw - mean * mean);
}

__global__ __launch_bounds__(256) void pt_denoise_atrous_kernel(const float4 *__restrict__ col_in, const float *__restrict__ var_in, const float4 *__restrict__ guide,
                                                                const uint32_t *__restrict__ cls, const float2 *__restrict__ grad, int32_t width, int32_t height,
                                                                int32_t step, float sigma_luminance, float sigma_normal, float sigma_depth,
                                                                float4 *__restrict__ col_out, float *__restrict__ var_out) {
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if(x >= width || y >= height) {
        return;
    }
    const int p = y * width + x;
    const uint32_t cp = cls[p];
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
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            g = g + k * var_in[qy * width + qx];
            gs = gs + k;
        }
    }
    g = g / gs;
    const float lum_scale = sigma_luminance * sqrtf(g) + kLumEps;
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
                if(sigma_luminance != 0.0f) {
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

// (rgba and out may be the same array: no __restrict__ on them)
__global__ __launch_bounds__(256) void pt_denoise_finish_kernel(const float4 *__restrict__ col, const float4 *rgba, const float4 *__restrict__ feat, int32_t width,
                                                                int32_t height, float4 *out) {
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if(x >= width || y >= height) {
        return;
    }
    const int p = y * width + x;
    const float4 f0 = feat[3 * p], f2 = feat[3 * p + 2];
    const float4 c = col[p];
    const float alpha = rgba[p].w;
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
    hipLaunchKernelGGL(pt_denoise_prepare_kernel, grid, block, 0, stream, rgba, features, width, height, s.col[0], s.guide, s.cls);
    hipLaunchKernelGGL(pt_denoise_variance_kernel, grid, block, 0, stream, s.col[0], s.guide, s.cls, width, height, params.sigma_normal, params.sigma_depth,
                       s.grad, s.var[0]);
    int cur = 0;
    for(int i = 0; i < params.iterations; i++) {
        hipLaunchKernelGGL(pt_denoise_atrous_kernel, grid, block, 0, stream, s.col[cur], s.var[cur], s.guide, s.cls, s.grad, width, height, 1 << i,
                           params.sigma_luminance, params.sigma_normal, params.sigma_depth, s.col[cur ^ 1], s.var[cur ^ 1]);
        cur ^= 1;
    }
    hipLaunchKernelGGL(pt_denoise_finish_kernel, grid, block, 0, stream, s.col[cur], rgba, features, width, height, out);
    return hipGetLastError();
}
