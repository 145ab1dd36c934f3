// pt_noise.h -- the rating of an unfinished pixel of a resumable frame (pt_frame_get_noise, pt_frame_set_noise_target)
// and the measured variance of its mean (pt_frame_get_variance), defined once for the kernels of pt_frame.hip.  Every operation is a correctly rounded fp32 operation in the order written here
// (tests/noise_ref.py restates it).
#ifndef PT_NOISE_H
#define PT_NOISE_H

#include <hip/hip_runtime.h>

#include "pt_types.h"

// the batch means the estimator has folded into contribution_mean / contribution_m2 (estimator_add, pt_shading.h)
__device__ inline int32_t pixel_batches(const PtEstimator &e, const PtDevOptions &opt) {
    return e.contribution_count / opt.stats_sample_count;
}

// The standard error of the pixel's mean, relative to what the reference's convergence test divides by: the reference's ratio
// stddev / (9 * get_contribution(mean) + floor) (worker.cpp:239-259, pt_shading.h:90-93; its floor is 1E-5) over the square root of the
// number of batch means.  +inf for a pixel with fewer than two batch means: it is unrated.  Never negative.
__device__ inline float pixel_error(const PtEstimator &e, const PtDevOptions &opt, float floor) {
    const int32_t batches = pixel_batches(e, opt);
    if(batches < 2) {
        return __builtin_inff();
    }
    const float d = (float)(batches - 1);
    const float r = e.contribution_m2[0] / d, g = e.contribution_m2[1] / d, b = e.contribution_m2[2] / d;
    const float stddev = __builtin_sqrtf(r + g + b);
    const float contribution = (e.contribution_mean[0] + e.contribution_mean[1] + e.contribution_mean[2]) / 3.0f; // get_contribution
    const float ratio = stddev / (9.0f * contribution + floor);
    return ratio / __builtin_sqrtf((float)batches);
}

// The measured variance of the pixel's mean, per channel, and the batch means behind it (pt_frame_get_variance): the sample
// variance of the B batch means over B, (v_r, v_g, v_b, (float)B).  A batch mean is the mean of stats_sample_count collected
// contributions, so v is in the unit of the preview colour pixel_value / collected_sample_count squared.  (0, 0, 0, 0) for a pixel with
// fewer than two batch means, or with a v_c that is negative, NaN or infinite: it is unrated.
__device__ inline float4 pixel_variance(const PtEstimator &e, const PtDevOptions &opt) {
    const int32_t batches = pixel_batches(e, opt);
    if(batches < 2) {
        return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const float d = (float)(batches - 1), n = (float)batches;
    const float r = (e.contribution_m2[0] / d) / n, g = (e.contribution_m2[1] / d) / n, b = (e.contribution_m2[2] / d) / n;
    const float top = 3.402823466e+38f;
    if(!(r >= 0.0f && r <= top && g >= 0.0f && g <= top && b >= 0.0f && b <= top)) {
        return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    return make_float4(r, g, b, n);
}

// the bin of an error in the 64-bin histogram by exponent: bin 32 = [1, 2), zero and the denormals in bin 0, 2^31 and above in bin 63
__device__ inline uint32_t pixel_error_bin(float error) {
    const int32_t b = (int32_t)((__float_as_uint(error) >> 23) & 0xffu) - 127 + 32;
    return (uint32_t)(b < 0 ? 0 : (b > 63 ? 63 : b));
}

#endif
