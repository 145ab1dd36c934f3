"""What a resumable view batch and the batched denoise cost, on the reference benchmark program's two scenes (Box, DragonBox
with the procedural stand-in mesh).

    python tools/views_frame_probe.py [--mesh-n 300] [--reps 3] [--scenes box,dragonbox] [--parts denoise,slices,preview]

denoise  batched denoise (B: render_features_views + denoise_views, one launch per stage) against the per-view loop it replaces (A:
         render_features + denoise per view), 64 views of 128^2 and 16 views of 256^2, same process, alternated; host wall time of the
         whole route (every call synchronises), median of `reps` after one warm-up of each.
slices   64 x 128^2 x 256 spp as a ViewsFrame in 1 call without a budget and under budgets giving about 4 and about 16 slices, against the
         uninterrupted process_views: device-event kernel time summed over the calls (pt_stats.kernel_ms), the calls, the largest drain_ms.
preview  the same batch after its first slice: wall time of the raw and the denoised preview (the calls synchronise), the first denoised
         preview apart (it runs the feature pass once), and the fraction of pixels with samples per view.
Prints one line per figure and a JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpupathtrace_amd import binding, scenes  # noqa: E402
from tools.views_probe import turntable  # noqa: E402


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def denoise_part(gpu, cam, reps):
    rows = []
    for n, size in ((64, 128), (16, 256)):
        opt = scenes.options(size, size, 4, 4)
        cams = turntable(cam, n)
        images = gpu.process_views(cams, opt, base_seeds=[1000 + v for v in range(n)])

        def loop():
            return np.stack([binding.denoise(images[v], gpu.render_features(cams[v], opt)) for v in range(n)])

        def batched():
            return binding.denoise_views(images, gpu.render_features_views(cams, opt))
        a0, b0 = loop(), batched()
        same = bool((a0.view(np.uint32) == b0.view(np.uint32)).all())
        a, b = [], []
        for _ in range(reps):
            a.append(wall(loop)[0])
            b.append(wall(batched)[0])
        rows.append({"views": n, "size": size, "loop_ms": statistics.median(a), "batched_ms": statistics.median(b), "bit_identical": same,
                     "loop_ms_all": a, "batched_ms_all": b})
        print("denoise  V=%-3d %3d^2  loop (A) %8.2f ms   batched (B) %8.2f ms   x%.2f   bit-identical %s" % (
            n, size, rows[-1]["loop_ms"], rows[-1]["batched_ms"], rows[-1]["loop_ms"] / rows[-1]["batched_ms"], same), flush=True)
    return rows


def run_frame(gpu, cams, opt, seeds, budget_ms):
    frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=seeds)
    try:
        kernel, calls, drain = 0.0, 0, 0.0
        t = time.perf_counter()
        while not frame.done:
            _, _, info = frame.render(budget_ms=budget_ms)
            kernel += sum(s["kernel_ms"] for s in info["stats"])
            drain = max(drain, info["drain_ms"])
            calls += 1
            assert calls < 500
        return {"budget_ms": budget_ms, "calls": calls, "kernel_ms": kernel, "wall_ms": (time.perf_counter() - t) * 1e3, "drain_ms": drain}
    finally:
        frame.close()


def slices_part(gpu, cam, reps):
    n, opt = 64, scenes.options(128, 128, 256, 256)
    cams, seeds = turntable(cam, n), [1000 + v for v in range(n)]
    gpu.process_views(cams, opt, base_seeds=seeds)
    base = statistics.median(gpu.process_views(cams, opt, base_seeds=seeds, want_stats=True)[1]["kernel_ms"] for _ in range(reps))
    print("slices   process_views, uninterrupted: kernel %8.2f ms" % base, flush=True)
    rows = [{"what": "process_views", "kernel_ms": base}]
    for what, budget in (("1 call", 0.0), ("~4 slices", base / 4.0), ("~16 slices", base / 16.0)):
        runs = [run_frame(gpu, cams, opt, seeds, budget) for _ in range(reps)]
        r = sorted(runs, key=lambda x: x["kernel_ms"])[len(runs) // 2]
        r["what"] = what
        rows.append(r)
        print("slices   %-10s budget %7.2f ms: %3d calls, kernel %8.2f ms (x%.3f), wall %8.2f ms, largest drain %.2f ms" % (
            what, budget, r["calls"], r["kernel_ms"], r["kernel_ms"] / base, r["wall_ms"], r["drain_ms"]), flush=True)
    return rows


def preview_part(gpu, cam, reps):
    n, opt = 64, scenes.options(128, 128, 256, 256)
    cams, seeds = turntable(cam, n), [1000 + v for v in range(n)]
    base = gpu.process_views(cams, opt, base_seeds=seeds, want_stats=True)[1]["kernel_ms"]
    frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=seeds)
    try:
        budget = base / 4.0
        for _ in range(20):
            _, _, info = frame.render(budget_ms=budget)
            if info["frame"]["streams_parked"] > 0 or frame.done:
                break
            budget *= 2.0
        first_denoised = wall(lambda: frame.preview(denoise=True))[0]
        raw = statistics.median(wall(frame.preview)[0] for _ in range(reps))
        den = statistics.median(wall(lambda: frame.preview(denoise=True))[0] for _ in range(reps))
        samples = frame.preview()[1]
        frac = [float((s != 0).mean()) for s in samples]
        r = {"frame": info["frame"], "raw_ms": raw, "denoised_ms": den, "first_denoised_ms": first_denoised, "features_once_ms": first_denoised - den,
             "fraction_with_samples": frac}
        print("preview  after the first slice (%d parked, %d finished, %d untouched): raw %.2f ms, denoised %.2f ms, first denoised %.2f ms "
              "(feature pass once: %.2f ms); views with samples everywhere %d of %d, least fraction %.3f" % (
                  info["frame"]["streams_parked"], info["frame"]["streams_finished"], info["frame"]["streams_untouched"], raw, den, first_denoised,
                  first_denoised - den, sum(f == 1.0 for f in frac), n, min(frac)), flush=True)
        return r
    finally:
        frame.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, default=300, help="stand-in mesh resolution (300 -> 179,400 triangles)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scenes", default="box,dragonbox")
    ap.add_argument("--parts", default="denoise,slices,preview")
    args = ap.parse_args()
    results = {}
    for name in args.scenes.split(","):
        if name == "box":
            sc, cam = scenes.box_scene()
        else:
            sc, cam = scenes.dragon_box_scene(*scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM))
        gpu = binding.Scene(sc, device=0)
        print("== %s" % name, flush=True)
        try:
            r = {}
            if "denoise" in args.parts:
                r["denoise"] = denoise_part(gpu, cam, args.reps)
            if "slices" in args.parts:
                r["slices"] = slices_part(gpu, cam, args.reps)
            if "preview" in args.parts:
                r["preview"] = preview_part(gpu, cam, args.reps)
            results[name] = r
        finally:
            gpu.close()
    print(json.dumps({"mesh_n": args.mesh_n, "reps": args.reps, "results": results}))


if __name__ == "__main__":
    main()
