"""numpy float32 restatement of the rating of an unfinished pixel (pixel_error, cpupathtrace_amd/csrc/pt_noise.h),
operation for operation: the batch statistics the estimator keeps (estimator_add, pt_shading.h: the Welford mean and M2 of the means of
batches of stats_sample_count collected samples), fed by the CPU oracle's get_sample as tests/preview_ref.py::raw_preview is, the error
made of them, and its histogram bin.  Every operation is one fp32 operation on float32 arrays, in the device code's order."""
import numpy as np

F = np.float32


def stats_sample_count(opt):
    """PtDevOptions::stats_sample_count (worker.cpp:158)"""
    return min(max(opt["min_sample_count"] // 4, 1), 64)


def batch_stats(checker, cam, opt, seed, xs, ys, draws, pixel_seed, seed_to_state):
    """The estimator's batch statistics of pixels (xs[i], ys[i]) after draws[i] samples: (contribution_count, contribution_mean (n, 4),
    contribution_m2 (n, 4), accepted).  accepted[i]: the estimator's own rule (worker.cpp:239-259, pt_shading.h:85-104) has finished the
    pixel within those samples; its statistics are then those at its last sample.  `checker` is an oracle scene handle; pixel_seed and
    seed_to_state are binding's."""
    xs, ys, draws = np.asarray(xs), np.asarray(ys), np.asarray(draws)
    w, h = opt["image_width"], opt["image_height"]
    per_batch = stats_sample_count(opt)
    half = F(0.5)
    xc = F(2) * ((xs.astype(F) + half) / F(w) - half)
    yc = -(F(2) * ((ys.astype(F) + half) / F(h) - half))
    xy = np.stack([xc, yc], axis=1).astype(F)
    states = np.array([seed_to_state(pixel_seed(seed, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
    n = len(xs)
    count = np.zeros(n, np.int32)
    index = np.zeros(n, np.int32)
    aggregate = np.zeros((n, 4), F)
    mean = np.zeros((n, 4), F)
    m2 = np.zeros((n, 4), F)
    check_count = min(max(opt["min_sample_count"] // 2, (opt["max_sample_count"] - opt["min_sample_count"]) // 8, 8, per_batch), 1024) // per_batch
    remaining = np.full(n, check_count, np.int32)
    accepted = np.zeros(n, bool)
    for j in range(int(draws.max()) if n else 0):
        act = np.nonzero((draws > j) & ~accepted)[0]
        if len(act) == 0:
            break
        rgba, col, st = checker.get_sample(cam, opt, xy[act], states[act])
        states[act] = st
        got = act[col != 0]
        count[got] += 1
        index[got] += 1
        aggregate[got] = aggregate[got] + rgba[col != 0].astype(F)
        full = got[index[got] == per_batch]
        agg = aggregate[full] / F(per_batch)
        delta = agg - mean[full]
        mean[full] = mean[full] + delta / (count[full] // per_batch).astype(F)[:, None]
        delta2 = agg - mean[full]
        m2[full] = m2[full] + delta * delta2
        index[full] = 0
        aggregate[full] = F(0)
        # the reference's convergence test, at a batch boundary once the pixel has its minimum of samples
        test = full[count[full] >= max(opt["min_sample_count"], 2)]
        batches = count[test] // per_batch
        with np.errstate(divide="ignore", invalid="ignore"):
            w = m2[test] / (batches - 1).astype(F)[:, None]
            stddev = np.sqrt((w[:, 0] + w[:, 1]) + w[:, 2])
            contribution = ((mean[test, 0] + mean[test, 1]) + mean[test, 2]) / F(3.0)
            ratio = stddev.astype(np.float64) / ((F(9.0) * contribution).astype(np.float64) + 1E-5)
        passed = (batches >= 2) & ((stddev < F(1E-4)) | (ratio < np.float64(F(0.2))))
        remaining[test[passed]] -= 1
        remaining[test[~passed]] = check_count
        accepted[test[passed & (remaining[test] <= 0)]] = True
    return count, mean, m2, accepted


def pixel_error(count, mean, m2, per_batch, floor=1e-5):
    """pixel_error of pt_noise.h over arrays: +inf where fewer than two batch means have been folded in (unrated)."""
    count = np.asarray(count, np.int32)
    mean, m2 = np.asarray(mean, F), np.asarray(m2, F)
    batches = count // np.int32(per_batch)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (batches - 1).astype(F)
        r, g, b = m2[..., 0] / d, m2[..., 1] / d, m2[..., 2] / d
        stddev = np.sqrt((r + g) + b)
        contribution = ((mean[..., 0] + mean[..., 1]) + mean[..., 2]) / F(3.0)
        ratio = stddev / (F(9.0) * contribution + F(floor))
        error = ratio / np.sqrt(batches.astype(F))
    assert error.dtype == F
    return np.where(batches < 2, F(np.inf), error).astype(F)


def error_bin(error):
    """pixel_error_bin of pt_noise.h: clamp(((bits >> 23) & 0xff) - 127 + 32, 0, 63)"""
    bits = np.asarray(error, F).view(np.uint32)
    return np.clip(((bits >> np.uint32(23)) & np.uint32(0xff)).astype(np.int64) - 127 + 32, 0, 63)


def oracle_error_map(checker, cam, opt, seed, xs, ys, draws, pixel_seed, seed_to_state, floor=1e-5):
    count, mean, m2, _ = batch_stats(checker, cam, opt, seed, xs, ys, draws, pixel_seed, seed_to_state)
    return pixel_error(count, mean, m2, stats_sample_count(opt), floor)


def summarise(error_map, target):
    """The summary pt_frame_get_noise gives, reduced from its error map: -1 finished, +inf unrated (a rated pixel's error is finite here),
    else rated; held = rated and error <= target > 0."""
    e = np.asarray(error_map, F).ravel()
    finished = e == F(-1)
    rated = ~finished & np.isfinite(e)
    unrated = ~finished & ~rated
    held = rated & (e <= F(target)) if target > 0 else np.zeros_like(rated)
    return {"streams_finished": int(finished.sum()), "streams_rated": int(rated.sum()), "streams_unrated": int(unrated.sum()), "streams_held": int(held.sum()),
            "max_error": F(e[rated].max()) if rated.any() else F(0), "histogram": np.bincount(error_bin(e[rated]), minlength=64).astype(np.uint32)}
