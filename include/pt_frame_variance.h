/* pt_frame_variance.h -- the measured variance of a resumable frame's unfinished pixels, and the preview's filter fed with it (DESIGN.md
 * 4.16).  Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h includes this file, which is not meant to be included on its own.
 *
 * Every unfinished pixel with a park record keeps the Welford mean and M2 of its B batch means (pt_frame_noise.h).  A batch mean is the mean
 * of stats_sample_count collected contributions, so it is in the unit of the preview colour (pixel_value / collected_sample_count), and the
 * variance of the pixel's mean is, per channel c = r, g, b and all in fp32 in this order:
 *     d   = (float)(B - 1)
 *     v_c = (m2.c / d) / (float)B
 *   - pt_frame_get_variance: the frame as it stands between two pt_frame_render calls, progressive or not; changes nothing.  out_var is
 *     [height][width][4] floats ([n_views][height][width][4] for a view frame): (v_r, v_g, v_b, (float)B) for a pixel with B >= 2 whose
 *     three v_c are finite and not negative -- a RATED pixel -- and (0, 0, 0, 0) for every other: unrated, finished, untouched or in no tile.
 *     Every replica gathers on its own device.  PT_ERR_INVALID for a null frame or map, or more than 0x0fffffff pixels; a failed frame returns
 *     its code.
 *   - pt_denoise_measured: pt_denoise (mask NULL) or the hole-aware filter of pt_frame_preview (mask: [height][width] int32, 0 = a hole) with
 *     such a plane, `variance`.  Where the plane's fourth component is >= 2 and its v_c are finite and not negative, the variance stage
 *     writes, in place of its 3x3 estimate,
 *         s_c = sqrtf(v_c) / max(albedo_c, 0.01)  on covered, non-emissive pixels (those the filter demodulates), sqrtf(v_c) on the others
 *         var = (0.2126 s_r + 0.7152 s_g + 0.0722 s_b)^2
 *     -- the channels taken as fully correlated: the estimator keeps no covariance between them -- and the pixel's luminance weight uses
 *     sigma_measured in place of sigma_luminance.  Everything else is pt_denoise's.  With a plane whose fourth component is 0 everywhere the
 *     result equals pt_denoise (or the hole-aware filter) bit for bit.  out_rgba may equal rgba.  The _device form works on DEVICE
 *     memory, ordered on `stream` (NULL = the default stream), which it synchronises before returning.  params NULL =
 *     pt_denoise_measured_params_default; sigma_measured 0 turns the luminance term off for rated pixels.  PT_ERR_INVALID before anything is
 *     uploaded or launched: a null rgba, features, variance or out_rgba, a size <= 0, more than 0x0fffffff pixels, parameters pt_denoise
 *     refuses, a negative or non-finite sigma_measured.
 *   - pt_frame_preview_measured: pt_frame_preview with denoising through this form and the frame's own variance map.  A complete frame has
 *     no rated pixel, so it previews as pt_frame_preview does.  Changes nothing the frame will do.  PT_ERR_INVALID as pt_frame_preview and
 *     for such parameters, before any device is touched; PT_ERR_UNSUPPORTED for a view frame. */
#ifndef PT_FRAME_VARIANCE_H
#define PT_FRAME_VARIANCE_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_denoise_measured_params {
    pt_denoise_params base;
    float sigma_measured; /* luminance edge-stopping of a rated pixel, in standard deviations of its measured luminance */
} pt_denoise_measured_params;
/* base = pt_denoise_params_default, sigma_measured 16: the best of a sweep on the Cornell box and the Box */
int pt_denoise_measured_params_default(pt_denoise_measured_params *out);
int pt_frame_get_variance(pt_frame *frame, float *out_var /* [H][W][4] */);
int pt_denoise_measured(int device, const float *rgba, const float *features, const float *variance, const int32_t *mask /* may be NULL */, int32_t width,
                        int32_t height, const pt_denoise_measured_params *params, float *out_rgba);
int pt_denoise_measured_device(int device, const float *d_rgba, const float *d_features, const float *d_variance, const int32_t *d_mask /* may be NULL */,
                               int32_t width, int32_t height, const pt_denoise_measured_params *params, float *d_out_rgba, void *stream);
int pt_frame_preview_measured(pt_frame *frame, const float *image, const pt_denoise_measured_params *params, float *out_rgba, int32_t *out_samples);

#ifdef __cplusplus
}
#endif

#endif
