"""Cost of the nearest-surface queries on the device: queries per second of pt_nearest_points_device and
pt_distance_grid_fill_device on scene L of tests/query_cases.py and on the benchmark scene (the DragonBox with its stand-in mesh), for
three workloads -- points drawn in the root box, points on the surface (what random rays hit) and a 64^3 grid over the root box --, with
the mean pair and leaf records a query's walk fetches (pt_debug_nearest_counts).  Figures are device events around the call on torch's
stream, the median of --repeats runs after one warm-up.  Nothing is compared: no earlier implementation exists.

    python tools/nearest_timing.py [--mesh-n 1900] [--points 1048576] [--grid 64] [--repeats 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--points", type=int, default=1 << 20, help="queries of the two point workloads")
    ap.add_argument("--grid", type=int, default=64, help="cells per axis of the grid workload")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cpupathtrace_amd import binding, scenes
    from tests import query_cases

    if binding.device_count() < 1:
        raise SystemExit("nearest_timing needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    stream = torch.cuda.current_stream()

    def device(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return statistics.median(out)

    def visits(gpu, q):
        counts, ms = np.zeros(2, np.uint64), C.c_float()
        binding._check(binding.load().pt_debug_nearest_counts(gpu._h, binding._ptr(q), C.c_size_t(len(q)), binding._ptr(counts), C.byref(ms)))
        return counts[0] / len(q), counts[1] / len(q)

    pos, nrm = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
    cases = [("scene L of tests/query_cases.py", query_cases.build(True)[0], (-1.0, -1.0, 0.0), (1.0, 1.0, 2.0), (0.0, 0.0, -1.0)),
             ("DragonBox, %d triangles" % len(pos), scenes.dragon_box_scene(pos, nrm, aspect_ratio=-1.0)[0], None, None, (0.5, 0.5, 0.5))]
    say("nearest_timing: device %s; median of %d runs" % (torch.cuda.get_device_name(0), args.repeats))
    for name, sc, lo, hi, eye in cases:
        gpu = binding.Scene(sc, device=0)
        try:
            rng = np.random.default_rng(0)
            n = args.points
            if lo is None:  # (a scene of plain triangles: the box of their corners)
                corners = np.asarray(sc["tri_pos"], np.float32).reshape(-1, 3)
                lo, hi = corners.min(axis=0), corners.max(axis=0)
            lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
            inside = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
            # points on the surface: what random rays from a place inside the scene hit
            d = rng.normal(size=(n, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            rays = np.concatenate([np.tile(np.asarray(eye, np.float64), (n, 1)), d], axis=1).astype(np.float32)
            hit = gpu.query(rays)
            surface = np.ascontiguousarray(np.resize(hit["position"][hit["object"] >= 0], (n, 3)), np.float32)
            info = gpu.info()
            say("%s: %d objects, tree depth %d" % (name, gpu.n_objects, info["depth"]))
            say("  %-22s %10s %10s %12s %12s %12s   %s" % ("workload", "queries", "ms", "Mqueries/s", "pairs/query", "leaves/query", "mean distance"))
            for label, points in (("in the root box", inside), ("on the surface", surface)):
                q = np.ascontiguousarray(np.concatenate([points, np.full((n, 1), np.inf, np.float32)], axis=1), np.float32)
                d_q = torch.from_numpy(q).to("cuda:0")
                d_out = torch.empty((n, 16), dtype=torch.int32, device="cuda:0")
                ms = device(lambda: gpu.nearest_device(d_q.data_ptr(), n, d_out.data_ptr(), stream.cuda_stream))
                pairs, leaves = visits(gpu, q)
                got = d_out.cpu().numpy().view(binding.Nearest).ravel()
                say("  %-22s %10d %10.3f %12.1f %12.1f %12.1f   %.4g" % (label, n, ms, n / ms / 1e3, pairs, leaves, float(got["distance"].mean())))
            g = args.grid
            grid = binding.distance_grid(lo, (hi - lo) / np.float32(max(g - 1, 1)), (g, g, g))
            d_distance = torch.empty((g, g, g), dtype=torch.float32, device="cuda:0")
            d_object = torch.empty((g, g, g), dtype=torch.int32, device="cuda:0")
            ms = device(lambda: gpu.distance_grid_device(grid, d_distance.data_ptr(), d_object.data_ptr(), np.inf, stream.cuda_stream))
            iz, iy, ix = np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij")
            idx = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1).astype(np.float32)
            nodes = np.ascontiguousarray(grid["origin"] + idx * grid["step"], np.float32)
            pairs, leaves = visits(gpu, np.ascontiguousarray(np.concatenate([nodes, np.full((len(nodes), 1), np.inf, np.float32)], axis=1), np.float32))
            say("  %-22s %10d %10.3f %12.1f %12.1f %12.1f   %.4g" % ("grid %d^3" % g, g ** 3, ms, g ** 3 / ms / 1e3, pairs, leaves, float(d_distance.mean())))
        finally:
            gpu.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
