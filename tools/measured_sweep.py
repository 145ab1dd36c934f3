"""Sweep of sigma_measured, the luminance sigma of the pixels whose variance is measured, on the numpy restatement
tests/denoise_measured_ref.py, the way DESIGN 4.10 chose sigma_luminance.  No GPU: the CPU oracle renders progressive frames bit for bit as
the device does (tests/test_gpu_frame_variance.py holds the device to it).

The frames (FRAME below; tests/test_gpu_frame_variance.py renders the same on the device): Cornell and Box at 128^2, min 16 / max 1024
samples, seed 1, progressive with quantum 16, stopped after the first pass -- the first after which every unfinished pixel is rated (16
samples: 4 batch means of 4).  The truth is 1024 spp of seed 99, relMSE is DESIGN 4.10's: mean over pixels and rgb of (x - g)^2 / (g^2 + 0.01).
The baseline is today's denoised preview at its defaults (tests/preview_ref.py).

    python tools/measured_sweep.py [--threads N] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import denoise_measured_ref as mr  # noqa: E402
from tests import denoise_ref, noise_ref, preview_ref  # noqa: E402

SIGMAS = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0)
FRAME = {"size": 128, "min_samples": 16, "max_samples": 1024, "seed": 1, "quantum": 16, "truth_samples": 1024, "truth_seed": 99}
F = np.float32


def relmse(x, g):
    x, g = x[..., :3].astype(np.float64), g[..., :3].astype(np.float64)
    return float(np.mean((x - g) ** 2 / (g ** 2 + 0.01)))


def scene_of(name):
    from cpupathtrace_amd import scenes
    n = FRAME["size"]
    sc, cam = scenes.cornell_scene(n, n) if name == "cornell" else scenes.box_scene()
    return sc, cam, scenes.options(n, n, FRAME["min_samples"], FRAME["max_samples"])


def stopped_frame(handle, cam, opt):
    """The stopped frame from the oracle: its raw preview, sample counts and variance map."""
    from cpupathtrace_amd import binding
    n = FRAME["size"]
    ys, xs = (a.ravel() for a in np.mgrid[0:n, 0:n])
    draws = np.full(n * n, FRAME["quantum"], np.int32)
    count, _, m2, accepted = noise_ref.batch_stats(handle, cam, opt, FRAME["seed"], xs, ys, draws, binding.pixel_seed, binding.seed_to_state)
    assert not accepted.any(), "no pixel finishes within the first pass"
    raw = preview_ref.raw_preview(handle, cam, opt, FRAME["seed"], xs, ys, draws, binding.pixel_seed, binding.seed_to_state)
    plane = mr.pixel_variance(count, m2, noise_ref.stats_sample_count(opt))
    return raw.reshape(n, n, 4), draws.reshape(n, n), plane.reshape(n, n, 4)


def truth_frame(handle, cam, threads):
    import oracle
    from cpupathtrace_amd import binding, scenes
    n = FRAME["size"]
    opt = scenes.options(n, n, FRAME["truth_samples"], FRAME["truth_samples"])
    ys, xs = (a.ravel() for a in np.mgrid[0:n, 0:n])
    states = np.array([binding.seed_to_state(binding.pixel_seed(FRAME["truth_seed"], int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
    image, _ = handle.render_streams(cam, opt, oracle.pixel_streams(xs, ys, states), n_threads=threads)
    return image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--out")
    args = ap.parse_args()
    import oracle
    oracle.build()
    chk = oracle.Checker("oracle")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("sigma_measured sweep: %s" % FRAME)
    for name in ("cornell", "box"):
        sc, cam, opt = scene_of(name)
        h = chk.scene_create(sc)
        try:
            raw, samples, plane = stopped_frame(h, cam, opt)
            feat = denoise_ref.host_features(chk, sc, cam, FRAME["size"], FRAME["size"])
            truth = truth_frame(h, cam, args.threads)
        finally:
            h.close()
        rated = mr.rated(plane)
        gm = truth[..., :3].astype(np.float64).mean(axis=(0, 1))
        say("%s: %d of %d pixels rated; relMSE raw preview %.5g; channel means raw %s, 1024 spp %s" % (
            name, rated.sum(), rated.size, relmse(raw, truth), raw[..., :3].astype(np.float64).mean(axis=(0, 1)), gm))
        base = preview_ref.denoise(raw, feat, samples, **denoise_ref.DEFAULTS)
        rb = relmse(base, truth)
        say("%s: existing preview denoise (sigma_luminance 32): relMSE %.5g; channel means %s" % (name, rb, base[..., :3].astype(np.float64).mean(axis=(0, 1))))
        for sm in SIGMAS:
            out = mr.denoise(raw, feat, plane, samples, **dict(denoise_ref.DEFAULTS, sigma_measured=sm))
            r = relmse(out, truth)
            say("%s: sigma_measured %4.1f: relMSE %.5g (ratio to the existing filter %.4f); channel means %s" % (
                name, sm, r, r / rb, out[..., :3].astype(np.float64).mean(axis=(0, 1))))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
