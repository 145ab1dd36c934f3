"""Parameter sweep of the temporal denoiser's defaults on the numpy restatement tests/temporal_ref.py, the way DESIGN 4.10
chose sigma_luminance.  The sequences are those of tests/test_gpu_temporal.py: 8 pushes of a static 128^2 camera at 16 spp (seeds 1..8) on the
Box and the Cornell box, and an orbit of 0.5 degrees per frame at 96^2 (seeds 1..8), with 1024-spp references.  They come from an .npz of
device renders (--frames; `--render` writes one on a GPU); every render is the CPU oracle's bit for bit (tests/test_gpu_parity.py), and
--oracle-check re-renders sample pixels of each static sequence with the oracle to show it.

    python tools/temporal_sweep.py --render FILE          (on a GPU: render the sequences)
    python tools/temporal_sweep.py --frames FILE [--oracle-check] [--out FILE]
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import denoise_ref, temporal_ref  # noqa: E402

SIGMA_LT = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0)
NORMAL_MIN = (0.8, 0.9, 0.95)
POSITION_TOL = (0.5, 1.0, 2.0, 4.0)


def orbit(cam, degrees):
    o, la = np.asarray(cam["origin"], np.float64), np.asarray(cam["look_at"], np.float64)
    a = math.radians(degrees)
    d = o - la
    rot = np.array([d[0] * math.cos(a) + d[2] * math.sin(a), d[1], -d[0] * math.sin(a) + d[2] * math.cos(a)])
    return dict(cam, origin=tuple(float(v) for v in la + rot))


def cameras(name, kind):
    from cpupathtrace_amd import scenes
    w = 128 if kind == "static" else 96
    sc, cam = scenes.cornell_scene(w, w) if name == "cornell" else scenes.box_scene()
    return sc, ([cam] * 8 if kind == "static" else [orbit(cam, 0.5 * k) for k in range(8)]), w


def render(path):
    from cpupathtrace_amd import binding, scenes
    out = {}
    for name in ("box", "cornell"):
        for kind in ("static", "orbit"):
            sc, cams, w = cameras(name, kind)
            gpu = binding.Scene(sc, device=0)
            try:
                opt = scenes.options(w, w, 16, 16)
                out["%s_%s_frames" % (name, kind)] = gpu.process_views(cams, opt, base_seeds=list(range(1, 9)))
                out["%s_%s_feat" % (name, kind)] = np.stack([gpu.render_features(c, opt) for c in cams])
                ref = scenes.options(w, w, 1024, 1024)
                if kind == "static":
                    out["%s_static_truth" % name] = gpu.process_job(cams[0], ref, base_seed=99)
                    out["%s_static_truth16k" % name] = gpu.process_job(cams[0], scenes.options(w, w, 16384, 16384), base_seed=97)
                else:
                    out["%s_orbit_truth" % name] = gpu.process_views(cams, ref, base_seeds=list(range(101, 109)))
            finally:
                gpu.close()
    np.savez_compressed(path, **out)


def oracle_check(data, say, n_pixels=48):
    """Sample pixels of every static frame, rendered by the oracle from the same per-pixel seeds, equal the device's bit for bit."""
    import oracle
    from cpupathtrace_amd import binding, scenes
    chk = oracle.Checker("oracle")
    rng = np.random.default_rng(0)
    for name in ("box", "cornell"):
        sc, cams, w = cameras(name, "static")
        frames = data["%s_static_frames" % name]
        handle = chk.scene_create(sc)
        for v in range(8):
            xs = rng.integers(0, w, n_pixels).astype(np.int32)
            ys = rng.integers(0, w, n_pixels).astype(np.int32)
            states = np.array([binding.seed_to_state(binding.pixel_seed(v + 1, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
            want, _ = handle.render_streams(cams[v], scenes.options(w, w, 16, 16), oracle.pixel_streams(xs, ys, states), n_threads=8)
            got = frames[v][ys, xs]
            same = (got.view(np.uint32) == want[ys, xs].view(np.uint32)).all()
            if not same:
                raise SystemExit("%s frame %d: the device render differs from the oracle" % (name, v))
        say("oracle check: %d sample pixels of each of the 8 static %s frames equal the oracle's bit for bit" % (n_pixels, name))


def relmse(x, g):
    x, g = x[..., :3].astype(np.float64), g[..., :3].astype(np.float64)
    return float(np.mean((x - g) ** 2 / (g ** 2 + 0.01)))


def run_sequence(frames, feats, cams, p):
    state = temporal_ref.TemporalState()
    outs, hist = [], []
    for v in range(len(cams)):
        out, n = temporal_ref.push(state, frames[v], feats[v], cams[v], p)
        outs.append(out)
        hist.append(n)
    return outs, hist


def flicker(outs, frames, feats, cams, hist, p):
    """Mean |out_v - out_{v-1} resampled with the denoiser's own taps| over pixels with n >= 2, frames 2..7."""
    d = []
    for v in range(2, len(cams)):
        c, l, _, cls, _ = denoise_ref.prepare(frames[v], feats[v])
        Xp, Np, _ = temporal_ref.surface(feats[v - 1])
        h, w = l.shape
        prev = {"cam": cams[v - 1], "col": np.zeros((h, w, 3), np.float32), "mom": np.zeros((h, w, 2), np.float32), "len": hist[v - 1],
                "pos": Xp, "nrm": Np, "cls": denoise_ref.prepare(frames[v - 1], feats[v - 1])[3]}
        _, _, _, n, taps, _ = temporal_ref.accumulate(c, l, cls, feats[v], cams[v], prev, p)
        back = temporal_ref.resample_previous(outs[v - 1][..., :3].astype(np.float64), taps)
        d.append(float(np.mean(np.abs(outs[v][..., :3] - back)[n >= 2])))
    return float(np.mean(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--render", default=None)
    ap.add_argument("--frames", default=None)
    ap.add_argument("--oracle-check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.render:
        render(args.render)
        return
    data = dict(np.load(args.frames))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.oracle_check:
        oracle_check(data, say)
    spatial_p = dict(denoise_ref.DEFAULTS)
    say("static camera, 128^2, 16 spp, 8 pushes: relMSE of the 8th output against 1024 spp (seed 99) and against 16384 spp (seed 97)")
    for name in ("box", "cornell"):
        _, cams, _ = cameras(name, "static")
        frames, feats = data["%s_static_frames" % name], data["%s_static_feat" % name]
        feat = feats[0] if feats.ndim == 5 else feats
        feats = [feat] * 8
        t1k, t16k = data["%s_static_truth" % name], data["%s_static_truth16k" % name]
        sp = denoise_ref.denoise(frames[7], feat, **spatial_p)
        floor = relmse(t1k, t16k)
        say("%s: the 1024-spp reference itself against 16384 spp: %.5g; noisy %.5g; spatial only %.5g (vs 16384 spp %.5g)" % (
            name, floor, relmse(frames[7], t1k), relmse(sp, t1k), relmse(sp, t16k)))
        rs = relmse(sp, t1k)
        for slt in SIGMA_LT:
            for ac in (0.2, 0.1):
                p = temporal_ref.params(sigma_luminance_temporal=slt, alpha_color=ac, alpha_moments=ac)
                outs, _ = run_sequence(frames, feats, cams, p)
                rt, rt16 = relmse(outs[7], t1k), relmse(outs[7], t16k)
                mean = outs[7][..., :3].astype(np.float64).mean(axis=(0, 1)) / t1k[..., :3].astype(np.float64).mean(axis=(0, 1)) - 1
                say("  sigma_lt %5.1f alpha %.1f: temporal %.5g (/ spatial %.3f); vs 16384 spp %.5g; channel means vs 1024 spp %s" % (
                    slt, ac, rt, rt / rs, rt16, np.round(mean * 100, 2)))
    say("orbit 0.5 deg/frame, 96^2, 16 spp: flicker (temporal / spatial) and mean relMSE frames 4..8 (temporal / spatial)")
    for name in ("cornell", "box"):
        _, cams, _ = cameras(name, "orbit")
        frames, feats, truths = data["%s_orbit_frames" % name], data["%s_orbit_feat" % name], data["%s_orbit_truth" % name]
        sp = [denoise_ref.denoise(frames[v], feats[v], **spatial_p) for v in range(8)]
        p0 = temporal_ref.params()
        _, hist0 = run_sequence(frames, feats, cams, p0)
        fs = flicker(sp, frames, feats, cams, hist0, p0)
        rs = float(np.mean([relmse(sp[v], truths[v]) for v in range(3, 8)]))
        for slt in (2.0, 4.0, 8.0):
            for nm in NORMAL_MIN:
                for tol in POSITION_TOL:
                    p = temporal_ref.params(sigma_luminance_temporal=slt, normal_min=nm, position_tolerance=tol)
                    outs, hist = run_sequence(frames, feats, cams, p)
                    ft = flicker(outs, frames, feats, cams, hist, p)
                    fs_p = flicker(sp, frames, feats, cams, hist, p)
                    rt = float(np.mean([relmse(outs[v], truths[v]) for v in range(3, 8)]))
                    kept = float(np.mean([(hist[v] >= 2).sum() / max(1, (hist[v] > 0).sum()) for v in range(1, 8)]))
                    say("  %s sigma_lt %4.1f normal_min %.2f tol %.1f: flicker %.3f, relMSE %.3f, pixels with history %.3f" % (
                        name, slt, nm, tol, ft / fs_p, rt / rs, kept))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
