/* pt_frame_noise.h -- the noise of a resumable frame and its noise target.  Part of the C ABI of libpathtrace_hip.so:
 * include/pt_hip.h includes this file, which is not meant to be included on its own.
 *
 * Every unfinished pixel of a frame that has a park record is RATED by the standard error of its mean, from the batch statistics its
 * estimator keeps anyway (B batch means of stats_sample_count samples each, their Welford mean and M2), all in fp32 in this order:
 *     stddev = sqrtf(m2.r / (B - 1) + m2.g / (B - 1) + m2.b / (B - 1))
 *     error  = (stddev / (9 * ((mean.r + mean.g + mean.b) / 3) + floor)) / sqrtf(B)
 * -- the ratio the reference's convergence test compares with 0.2 (worker.cpp:239-259, floor 1E-5), over sqrt(B), so that it falls as the
 * pixel takes samples.  A pixel with B < 2 is UNRATED.  With floor = 0 a pixel whose samples are all black rates NaN, which no target holds
 * (0 / 0 on the device: the pattern 0xffc00000).  A rated pixel whose M2 has overflowed rates +inf and is not held either.
 *   - pt_frame_get_noise: the frame as it stands between two pt_frame_render calls, progressive or not; changes nothing.  The summary counts
 *     the unfinished streams (rated + unrated = streams_total - streams_finished; untouched streams are unrated), those a target would hold
 *     (rated, target_error > 0 and error <= target_error), the largest error and a histogram of the rated streams by the exponent of their
 *     error: bin = clamp(exponent - 127 + 32, 0, 63), so bin 32 is [1, 2) and an error of 0 is in bin 0; +inf and NaN are in bin 63.  All
 *     of it is reduced with integer operations: it does not depend on the order of execution.  max_error is the largest BIT PATTERN of a
 *     rated stream's error, taken as an unsigned word: the largest error where every rated error is a number or +inf, and NaN as soon
 *     as one rated stream rates NaN (a NaN's pattern is above +inf's).  out_error (may be NULL; [height][width], or [n_views][height][width] for a
 *     view frame): -1 for a finished pixel, +inf for an unrated or untouched pixel and a pixel of no tile, else the error.
 *     PT_ERR_INVALID for a null frame or summary, or more than 0x0fffffff pixels.
 *   - pt_frame_set_noise_target: only between two pt_frame_render calls.  target_error 0 turns the target off; floor and fraction are kept
 *     for pt_frame_get_noise either way.  PT_ERR_INVALID, before any device is touched, for a null frame, a negative or non-finite
 *     target_error or floor, or a fraction outside (0, 1]; a failed frame returns its code.
 *   - A PROGRESSIVE frame (pt_frame_set_progressive) with a target HOLDS every stream whose error is at or below the target: a pass does not
 *     claim it, it takes no samples, and its record is carried to the pass's records like that of a stream the launch never reached.  What
 *     is held is decided from the records before every pass and stored nowhere: a lower target (or none) releases streams in the next
 *     pass, a higher one holds more.  A pass is complete when every unfinished stream has the pass's samples or is held.  Before a new pass
 *     pt_frame_render compares (double)(finished + held) with (double)fraction * (double)streams_total: once it is not less, the call
 *     returns PT_ERR_CANCELLED with "noise target reached" in pt_last_error, and every later call does so at once, without a launch, until
 *     pt_frame_set_noise_target is called again.  Such a frame is stopped, not complete: its picture is its pt_frame_preview.  Held streams
 *     are parked streams (pt_frame_info::streams_parked) and no sample is ever lost.  A plain frame ignores the target.
 *   - Clear the target and render on: the finished frame is bit-identical to pt_render_tiles / pt_render_views with the same arguments,
 *     whatever targets, quanta and stops came before -- every pixel still runs its own engine through the same chain of samples. */
#ifndef PT_FRAME_NOISE_H
#define PT_FRAME_NOISE_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_frame_noise {
    float target_error, floor, fraction;   /* as set; target_error 0 = no target */
    int32_t target_reached;                /* 1 = finished + held >= fraction * streams_total */
    uint64_t streams_total, streams_finished, streams_rated, streams_unrated, streams_held;
    float max_error;                       /* over rated streams, 0 if none; NaN if one of them rates NaN (see above) */
    uint32_t histogram[64];                /* rated streams by exponent of their error */
} pt_frame_noise;
int pt_frame_get_noise(pt_frame *frame, pt_frame_noise *out, float *out_error /* [H][W] or [V][H][W], may be NULL */);
int pt_frame_set_noise_target(pt_frame *frame, float target_error, float floor, float fraction);

#ifdef __cplusplus
}
#endif

#endif
