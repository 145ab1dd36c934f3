"""Msamples/s of a batch of V views (Scene.process_views: one launch) against the same V views rendered one process_job call after another,
on the reference benchmark program's two scenes (benchmark/main.cpp: renderSceneBox, renderSceneDragonBox with the procedural stand-in mesh),
128 x 128 x 256 spp (min = max) per view by default.

    python tools/views_probe.py [--views 1,4,16,64] [--size 128] [--spp 256] [--mesh-n 300] [--reps 3] [--scenes box,dragonbox]

Times are device-event times of the launches (pt_stats.kernel_ms: HIP events around each launch on the library's stream), summed over the V
launches of the separate calls; wall-clock times of the whole calls are printed next to them.  Every configuration is warmed up once (one
batch and one single call) and then measured `reps` times, alternating batch and separate; the median is reported.  Views are a turntable
around the scene's camera, view v seeded with 1000 + v.  Prints one line per configuration and a JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpupathtrace_amd import binding, scenes  # noqa: E402


def turntable(cam, n):
    """n cameras on a circle of the camera's distance around the look-at point (same up, same lens)."""
    o, c = np.array(cam["origin"], float), np.array(cam["look_at"], float)
    r = o - c
    out = []
    for v in range(n):
        a = 2.0 * np.pi * v / max(n, 1) * 0.25  # a quarter turn: every view still looks into the open side of the box
        rot = np.array([r[0] * np.cos(a) + r[2] * np.sin(a), r[1], -r[0] * np.sin(a) + r[2] * np.cos(a)])
        out.append(dict(cam, origin=tuple(float(x) for x in c + rot)))
    return out


def measure(gpu, cams, opt, reps):
    seeds = [1000 + v for v in range(len(cams))]
    pixels = opt["image_width"] * opt["image_height"]
    gpu.process_views(cams, opt, base_seeds=seeds)  # warm-up: the workspace of both job sizes exists before anything is timed
    gpu.process_job(cams[0], opt, base_seed=seeds[0])
    batch, batch_wall, single, single_wall, samples = [], [], [], [], 0
    for _ in range(reps):
        t = time.perf_counter()
        _, st = gpu.process_views(cams, opt, base_seeds=seeds, want_stats=True)
        batch_wall.append(time.perf_counter() - t)
        batch.append(st["kernel_ms"])
        samples = st["samples"]
        ms, t = 0.0, time.perf_counter()
        for c, s in zip(cams, seeds):
            _, st1 = gpu.process_job(c, opt, base_seed=s, want_stats=True)
            ms += st1["kernel_ms"]
        single_wall.append(time.perf_counter() - t)
        single.append(ms)
    assert samples == len(cams) * pixels * opt["max_sample_count"], samples
    b, s = statistics.median(batch), statistics.median(single)
    return {"views": len(cams), "samples": samples, "batch_ms": b, "separate_ms": s, "batch_msps": samples / b / 1e3, "separate_msps": samples / s / 1e3,
            "speedup": s / b, "batch_wall_s": statistics.median(batch_wall), "separate_wall_s": statistics.median(single_wall),
            "batch_ms_all": batch, "separate_ms_all": single}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="1,4,16,64")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--mesh-n", type=int, default=300, help="stand-in mesh resolution (300 -> 179,400 triangles)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scenes", default="box,dragonbox")
    args = ap.parse_args()
    opt = scenes.options(args.size, args.size, args.spp, args.spp)
    results = []
    for name in args.scenes.split(","):
        if name == "box":
            sc, cam = scenes.box_scene()
        else:
            sc, cam = scenes.dragon_box_scene(*scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM))
        gpu = binding.Scene(sc, device=0)
        try:
            for n in [int(v) for v in args.views.split(",")]:
                r = measure(gpu, turntable(cam, n), opt, args.reps)
                r["scene"] = name
                results.append(r)
                print("%-9s V=%-3d  batch %8.2f ms %7.1f Msamples/s   separate %8.2f ms %7.1f Msamples/s   x%.2f   (wall %.3f s / %.3f s)" % (
                    name, n, r["batch_ms"], r["batch_msps"], r["separate_ms"], r["separate_msps"], r["speedup"], r["batch_wall_s"], r["separate_wall_s"]),
                    flush=True)
        finally:
            gpu.close()
    print(json.dumps({"size": args.size, "spp": args.spp, "mesh_n": args.mesh_n, "reps": args.reps, "results": results}))


if __name__ == "__main__":
    main()
