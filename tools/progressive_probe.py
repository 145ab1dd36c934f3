"""What a progressive pass costs: renders a workload once uninterrupted (process_job / process_views), then as a progressive frame
(binding.Frame.set_progressive) pass by pass for each schedule of quanta, and prints per schedule the passes it took, the kernel time summed
over them against the uninterrupted render's, the time per pass, the park records moved per pass (every stream left reads and writes one
528-byte record), the park storage, the preview's coverage after pass 1 and whether the frame is bit-identical.

    python tools/progressive_probe.py [--workload metric|box1080|views] [--spp 64] [--schedules 16,64,doubling] [--mesh-n 1900]

metric: the benchmark frame (DragonBox, 1024 x 1024); box1080: the Box scene at 1920 x 1080; views: 64 views of 128 x 128 of the Box scene.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cpupathtrace_amd import binding, scenes  # noqa: E402

SEED = 1234
RECORD_BYTES = 528


def quanta(schedule):
    if schedule == "doubling":
        yield 1
        q = 1
        while True:
            yield q
            q *= 2
    while True:
        yield int(schedule)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="box1080", choices=["metric", "box1080", "views"])
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--schedules", default="16,64,doubling")
    args = ap.parse_args()
    views = None
    if args.workload == "metric":
        w = h = 1024
        sc, cam = scenes.dragon_box_scene(*scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM), aspect_ratio=-1.0)
    elif args.workload == "box1080":
        w, h = 1920, 1080
        sc, cam = scenes.box_scene(aspect_ratio=-float(np.float32(w) / np.float32(h)))
    else:
        w = h = 128
        sc, cam = scenes.box_scene()
        views = []
        for v in range(64):
            c = dict(cam)
            a = 2.0 * np.pi * v / 64
            c["origin"] = (float(3.0 * np.sin(a) * 0.2), 0.1 * np.cos(a), -3.0 + 0.2 * (1.0 - np.cos(a)))
            views.append(c)
    gpu = binding.Scene(sc, device=0)
    opt = scenes.options(w, h, args.spp, args.spp)
    gpu.process_job(cam, scenes.options(64, 64, 4, 4))  # (warm-up: workspace and code object)
    if views is None:
        full, st = gpu.process_job(cam, opt, base_seed=SEED, want_stats=True)
    else:
        full, st = gpu.process_views(views, opt, base_seeds=SEED, want_stats=True)
    print("%s %dx%d%s %d spp uninterrupted: kernel %.1f ms" % (args.workload, w, h, " x %d views" % len(views) if views else "", args.spp, st["kernel_ms"]), flush=True)
    for schedule in args.schedules.split(","):
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED) if views is None else binding.ViewsFrame(gpu, views, opt, base_seeds=SEED)
        per_pass, moved, coverage, park_bytes = [], [], None, 0
        t0 = time.perf_counter()
        for q in quanta(schedule):
            frame.set_progressive(q, 1)
            before = frame.info()
            img, _, info = frame.render()
            per_pass.append(sum(s["kernel_ms"] for s in info["stats"]))
            # records read (the streams that came in parked) and written (the streams that left parked)
            moved.append((before["streams_parked"] + info["frame"]["streams_parked"]) * RECORD_BYTES)
            park_bytes = max(park_bytes, info["frame"]["park_bytes"])
            if coverage is None:
                coverage = float((frame.preview()[1] != 0).mean())
            if info["status"] == binding.PT_OK:
                break
        wall = (time.perf_counter() - t0) * 1e3
        kernel = sum(per_pass)
        same = bool((img.view(np.uint32) == full.view(np.uint32)).all())
        print("quantum %s: %d passes, kernel %.1f ms (%+.1f ms, %+.1f %%), %.2f ms per pass on average (first %.2f, last %.2f), wall %.1f ms; park records moved per pass "
              "%.1f MiB on average; park storage %.1f MiB; coverage after pass 1 %.3f; bit-identical %s" % (
                  schedule, len(per_pass), kernel, kernel - st["kernel_ms"], 100.0 * (kernel / st["kernel_ms"] - 1.0), kernel / len(per_pass), per_pass[0], per_pass[-1],
                  wall, np.mean(moved) / 2**20, park_bytes / 2**20, coverage, same), flush=True)
        frame.close()
    gpu.close()


if __name__ == "__main__":
    main()
