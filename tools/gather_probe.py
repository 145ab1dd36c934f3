"""Cost of the gathers on the device: samples per second of pt_gather_points_device for each kind -- occlusion, direct
light, whole paths -- on the benchmark scene (the DragonBox with its stand-in mesh) and on the Box scene, for many points x few samples
and for few points x many samples, beside the path kernel's samples per second on the same scene (process_job's own count of samples
over its kernel time).  The points are what 65 536 random rays from a place inside the scene hit, with the normals turned against the
rays, repeated to the count asked for.  Gather figures are device events around the call on torch's stream -- gather kernels and the
ordered reduce, every chunk --, and beside them the host's clock around the call and a device synchronise; each the median of --repeats
runs after one warm-up.  The mean value over the points is printed as a check that the samples found something to gather.

    python tools/gather_probe.py [--mesh-n 1900] [--many 262144x4] [--few 1024x1024] [--size 512] [--distance 0.5] [--origin X Y Z] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shape(text):
    points, samples = text.lower().split("x")
    return int(points), int(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--many", type=shape, default=(1 << 18, 4), help="points x samples of the many-points case")
    ap.add_argument("--few", type=shape, default=(1 << 10, 1 << 10), help="points x samples of the many-samples case")
    ap.add_argument("--size", type=int, default=512, help="side of the frame of the path kernel's figure")
    ap.add_argument("--spp", type=int, default=16, help="samples per pixel of the path kernel's frame")
    ap.add_argument("--distance", type=float, default=0.5, help="occlusion distance (both scenes are boxes of side 2)")
    ap.add_argument("--origin", type=float, nargs=3, default=(0.5, 0.5, 0.5), help="where the rays that find the points start: inside the box, outside the mesh")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cpupathtrace_amd import binding, scenes

    if binding.device_count() < 1:
        raise SystemExit("gather_probe needs a GPU")
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

    def wall(fn):
        """host clock around the call and a device synchronise"""
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    pos, nrm = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
    cases = [("DragonBox, %d triangles" % len(pos), scenes.dragon_box_scene(pos, nrm, aspect_ratio=-1.0)), ("Box", scenes.box_scene(aspect_ratio=-1.0))]
    say("gather_probe: device %s; median of %d runs; occlusion distance %g" % (torch.cuda.get_device_name(0), args.repeats, args.distance))
    for name, (sc, cam) in cases:
        gpu = binding.Scene(sc, device=0)
        try:
            w = args.size
            opt = scenes.options(w, w, args.spp, args.spp)
            # points inside the scene: what random rays from a place inside it hit, the normals turned against them
            rng = np.random.default_rng(0)
            d = rng.normal(size=(1 << 16, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            rays = np.concatenate([np.tile(np.asarray(args.origin, np.float64), (len(d), 1)), d], axis=1).astype(np.float32)
            hit = gpu.query(rays)
            rays, hit = rays[hit["object"] >= 0], hit[hit["object"] >= 0]
            normal = np.where(((hit["normal"] * rays[:, 3:]).sum(axis=1) > 0)[:, None], -hit["normal"], hit["normal"])
            points = np.ascontiguousarray(np.concatenate([hit["position"], normal], axis=1), np.float32)
            distance = args.distance
            _, stats = gpu.process_job(cam, opt, base_seed=1, want_stats=True)
            _, stats = gpu.process_job(cam, opt, base_seed=1, want_stats=True)
            say("%s: %d distinct points; path kernel %d x %d x %d spp: %.2f ms, %.1f Msamples/s" % (
                name, len(hit), w, w, args.spp, stats["kernel_ms"], stats["samples"] / stats["kernel_ms"] / 1e3))
            say("  %-12s %10s %8s %10s %10s %14s   %s" % ("kind", "points", "samples", "ms", "wall ms", "Msamples/s", "mean value"))
            for n, samples in (args.many, args.few):
                pts = np.ascontiguousarray(np.resize(points, (n, 6)))
                d_pts = torch.from_numpy(pts).to("cuda:0")
                d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
                for kind, kind_name in ((binding.GATHER_OCCLUSION, "occlusion"), (binding.GATHER_DIRECT, "direct"), (binding.GATHER_PATHS, "paths")):
                    call = lambda: gpu.gather_device(d_pts.data_ptr(), n, d_out.data_ptr(), kind, samples, opt["epsilon"], distance, 1, stream.cuda_stream)
                    ms, wall_ms = device(call), wall(call)
                    got = d_out.cpu().numpy().view(binding.GatherResult).ravel()
                    say("  %-12s %10d %8d %10.2f %10.2f %14.1f   %s" % (kind_name, n, samples, ms, wall_ms, n * samples / ms / 1e3, np.array2string(got["value"][:, :3].mean(axis=0), precision=4)))
        finally:
            gpu.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
