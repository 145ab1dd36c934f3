"""What resuming costs: renders a benchmark frame once uninterrupted (process_job), then as a resumable frame (binding.Frame) in slices of
wall-clock budget full / N for each N, and prints per N the calls it took, the kernel time summed over them against the uninterrupted
frame's, the park storage and whether the frame is bit-identical.  Total kernel time is what the device spent, excluding the host's part
of a call (uploads, the poll loop).

    python tools/frame_slice_probe.py [--workload dragon|box] [--size 1024] [--spp 1024] [--slices 1,4,16]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="dragon", choices=["dragon", "box"])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--slices", default="1,4,16", help="comma-separated slice counts")
    args = ap.parse_args()
    aspect = -float(np.float32(args.size) / np.float32(args.size))
    if args.workload == "dragon":
        pos, nrm = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
        sc, cam = scenes.dragon_box_scene(pos, nrm, aspect_ratio=aspect)
    else:
        sc, cam = scenes.box_scene(aspect_ratio=aspect)
    gpu = binding.Scene(sc, device=0)
    opt = scenes.options(args.size, args.size, args.spp, args.spp)
    gpu.process_job(cam, scenes.options(64, 64, 4, 4))  # (warm-up: workspace and code object)
    t0 = time.perf_counter()
    full, st = gpu.process_job(cam, opt, base_seed=SEED, want_stats=True)
    full_wall = (time.perf_counter() - t0) * 1e3
    print("%s %dx%d %d spp uninterrupted: kernel %.1f ms, wall %.1f ms" % (args.workload, args.size, args.size, args.spp, st["kernel_ms"], full_wall), flush=True)
    for n in [int(x) for x in args.slices.split(",")]:
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        budget = 0.0 if n <= 1 else full_wall / n
        kernel, calls, parked, drains, park_bytes = 0.0, 0, [], [], 0
        t0 = time.perf_counter()
        while not frame.done and calls < 100 * max(n, 1):
            img, _, info = frame.render(budget_ms=budget)
            calls += 1
            kernel += sum(s["kernel_ms"] for s in info["stats"])
            parked.append(info["streams_abandoned"])
            drains.append(info["drain_ms"])
            park_bytes = max(park_bytes, info["frame"]["park_bytes"])
        wall = (time.perf_counter() - t0) * 1e3
        same = bool((img.view(np.uint32) == full.view(np.uint32)).all())
        print("slices of %s: %d calls, kernel %.1f ms (%+.1f ms, %+.1f ms per stopped call), wall %.1f ms; park storage %.1f MiB; parked per call %s; "
              "drain per call %s ms; bit-identical %s" % (
                  "%.1f ms" % budget if budget else "no budget", calls, kernel, kernel - st["kernel_ms"], (kernel - st["kernel_ms"]) / max(calls - 1, 1), wall,
                  park_bytes / 2**20, parked, ["%.1f" % d for d in drains], same), flush=True)
        frame.close()
    gpu.close()


if __name__ == "__main__":
    main()
