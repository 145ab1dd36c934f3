"""What followed features do to the denoised frame, measured on the CPU: the oracle renders the frames -- bit for bit as
the device does -- tests/denoise_ref.py filters them at its defaults, once with the first-hit features (tests/denoise_ref.host_features)
and once with the followed ones (tests/features_follow_ref.followed_features).  No GPU.

The frames (features_follow_ref.QUALITY; tests/test_gpu_features_follow.py renders the same on the device): cornell_scene and
advanced_scene at 96^2, 16 spp of seed 1 against 1024 spp of seed 99.  S: the pixels with a primary ray whose first hit is glass or a
mirror; relMSE is DESIGN 4.10's, over S and over the rest.  The two ratios followed / first-hit per scene are what the GPU test asserts,
widened by 10 %.

    python tools/follow_sweep.py [--threads N] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import denoise_ref  # noqa: E402
from tests import features_follow_ref as ffr  # noqa: E402


def frame(handle, cam, samples, seed, threads):
    import oracle
    from cpupathtrace_amd import binding, scenes
    n = ffr.QUALITY["size"]
    opt = scenes.options(n, n, samples, samples, epsilon=ffr.QUALITY["epsilon"])
    ys, xs = (a.ravel() for a in np.mgrid[0:n, 0:n])
    states = np.array([binding.seed_to_state(binding.pixel_seed(seed, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
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

    q = ffr.QUALITY
    n = q["size"]
    say("followed features, measured on the CPU (oracle frames, numpy filter): %s" % q)
    for name in ("cornell", "advanced"):
        sc, cam = ffr.quality_scene(name)
        h = chk.scene_create(sc)
        try:
            noisy = frame(h, cam, q["samples"], q["seed"], args.threads)
            truth = frame(h, cam, q["truth_samples"], q["truth_seed"], args.threads)
        finally:
            h.close()
        in_s = ffr.first_hit_specular(chk, sc, cam, n, n) > 0
        first = denoise_ref.denoise(noisy, denoise_ref.host_features(chk, sc, cam, n, n), **denoise_ref.DEFAULTS)
        followed = denoise_ref.denoise(noisy, ffr.followed_features(chk, sc, cam, n, n, q["max_bounces"], q["epsilon"]), **denoise_ref.DEFAULTS)
        everywhere = np.ones_like(in_s)
        say("%s: %d of %d pixels in S" % (name, in_s.sum(), in_s.size))
        for what, where in (("S", in_s), ("rest", ~in_s), ("whole frame", everywhere)):
            rn, rf, ro = (ffr.relmse_on(x, truth, where) for x in (noisy, first, followed))
            say("%s: relMSE on %s: noisy %.5g, first-hit features %.5g, followed %.5g; ratio followed / first-hit %.4f" % (name, what, rn, rf, ro, ro / rf))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
