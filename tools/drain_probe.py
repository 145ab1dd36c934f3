"""How quickly a stop takes effect: renders a benchmark frame under a wall-clock budget (pt_render_tiles_ctl) and prints, per budget, when the
call returned, drain_ms (from the stop request to the end of the launch, as the host saw it) and what became of the streams.

    python tools/drain_probe.py [--workload dragon|box] [--size 1024] [--spp 1024] [--budgets 500,1000]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cpupathtrace_amd import binding, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="dragon", choices=["dragon", "box"])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--budgets", default="500,1000", help="comma-separated budgets in ms")
    args = ap.parse_args()
    aspect = -float(np.float32(args.size) / np.float32(args.size))
    if args.workload == "dragon":
        pos, nrm = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
        sc, cam = scenes.dragon_box_scene(pos, nrm, aspect_ratio=aspect)
    else:
        sc, cam = scenes.box_scene(aspect_ratio=aspect)
    gpu = binding.Scene(sc, device=0)
    opt = scenes.options(args.size, args.size, args.spp, args.spp)
    gpu.process_job_controlled(cam, scenes.options(64, 64, 4, 4))  # (warm-up: workspace and code object)
    for budget in [float(b) for b in args.budgets.split(",")]:
        t0 = time.perf_counter()
        _, tile_done, info = gpu.process_job_controlled(cam, opt, budget_ms=budget)
        wall = (time.perf_counter() - t0) * 1e3
        st = info["stats"][0]
        print("%s %dx%d %d spp, budget %.0f ms: returned after %.1f ms, kernel %.1f ms, drain %.2f ms; status %d, tiles %d of %d, streams finished %d "
              "abandoned %d unclaimed %d" % (args.workload, args.size, args.size, args.spp, budget, wall, st["kernel_ms"], info["drain_ms"], info["status"],
                                             tile_done.sum(), len(tile_done), info["streams_finished"], info["streams_abandoned"], info["streams_unclaimed"]),
              flush=True)
    gpu.close()


if __name__ == "__main__":
    main()
