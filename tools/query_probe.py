"""Cost of the scene queries on the device: rays per second of pt_query_rays and pt_occluded_rays next to
pt_intersect_batch -- whose kernel and host loop the queries leave untouched -- on the benchmark scene (the DragonBox with its stand-in
mesh), and the time of a 1024^2 pt_query_frame next to pt_render_features, which traces four rays per pixel.  Host forms are wall time
around the call (uploads, downloads and pt_intersect_batch's host loop included); device forms are device events around the call on
torch's stream.  Every figure is the median of --repeats runs after one warm-up.

    python tools/query_probe.py [--mesh-n 1900] [--rays 4194304] [--size 1024] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cpupathtrace_amd import binding, scenes

    if binding.device_count() < 1:
        raise SystemExit("query_probe needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def wall(fn):
        fn()
        out = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

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

    pos, nrm = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
    sc, cam = scenes.dragon_box_scene(pos, nrm, aspect_ratio=-1.0)
    gpu = binding.Scene(sc, device=0)
    try:
        n = args.rays
        rng = np.random.default_rng(0)
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.concatenate([rng.uniform(-0.9, 0.9, (n, 3)), d], axis=1).astype(np.float32)
        t, _ = gpu.get_intersection(rays)
        hit = t >= 0
        # shadow-like segments: half of the hitting rays stop short of their hit (not blocked), half go on past it (blocked)
        t_max = np.where(np.arange(n) % 2 == 0, 0.5 * t, 2.0 * t).astype(np.float32)
        t_max[~hit] = np.inf
        seg = np.concatenate([rays, t_max[:, None]], axis=1).astype(np.float32)
        say("query_probe: device %s; %d triangles; %d rays, %.1f %% hit; median of %d runs" % (torch.cuda.get_device_name(0), len(pos), n, 100 * hit.mean(), args.repeats))
        say("%-34s %10s %12s" % ("call", "ms", "Mrays/s"))

        def row(name, ms, count=n):
            say("%-34s %10.2f %12.1f" % (name, ms, count / ms / 1e3))

        row("pt_intersect_batch (host)", wall(lambda: gpu.get_intersection(rays)))
        row("pt_query_rays (host)", wall(lambda: gpu.query(rays)))
        row("pt_occluded_rays (host)", wall(lambda: gpu.occluded(rays, t_max)))
        d_rays, d_seg = torch.from_numpy(rays).to("cuda:0"), torch.from_numpy(seg).to("cuda:0")
        d_hits = torch.empty((n, 16), dtype=torch.float32, device="cuda:0")
        d_flags = torch.empty((n,), dtype=torch.uint8, device="cuda:0")
        s = stream.cuda_stream
        row("pt_query_rays_device", device(lambda: gpu.query_device(d_rays.data_ptr(), n, d_hits.data_ptr(), s)))
        row("pt_occluded_rays_device", device(lambda: gpu.occluded_device(d_seg.data_ptr(), n, d_flags.data_ptr(), s)))
        d_seg[:, 6] = float("inf")
        row("pt_occluded_rays_device, t_max inf", device(lambda: gpu.occluded_device(d_seg.data_ptr(), n, d_flags.data_ptr(), s)))
        blocked = int(d_flags.sum().item())
        say("(with t_max = inf %d of %d segments are blocked: every ray that hits)" % (blocked, n))
        w = args.size
        opt = scenes.options(w, w, 1, 1)
        cam = dict(cam, aspect_ratio=-1.0)
        d_frame = torch.empty((w * w, 16), dtype=torch.float32, device="cuda:0")
        d_feat = torch.empty((w, w, 3, 4), dtype=torch.float32, device="cuda:0")
        say("%-34s %10s %12s" % ("%d x %d frame" % (w, w), "ms", "Mrays/s"))
        row("pt_query_frame_device", device(lambda: gpu.id_map_device(cam, opt, d_frame.data_ptr(), s)), w * w)
        row("pt_render_features_device (4 rays)", device(lambda: gpu.render_features_device(cam, opt, d_feat.data_ptr(), s)), 4 * w * w)
    finally:
        gpu.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
