"""Cost of the light probes on the device: samples per second of pt_light_probes_points_device on the benchmark scene (the
DragonBox with its stand-in mesh) and on the Box scene for many probes x few samples, few probes x many samples and a grid, each beside
pt_gather_points_device with PT_GATHER_PATHS at the same pair count in the same run (different workloads, set side by side: a probe's
first ray starts in free space and goes anywhere, a gather's starts on a surface and goes into its hemisphere); a bound on the projection
kernel's share of a call: the time of the same call with probes far outside the scene, whose samples all miss at the root box -- the
sampling kernel at its cheapest and the same projection --, over the time of the call inside the scene; and the lookup's rate for 1 Mi
points.  Figures are device events around the call on torch's stream, the median of --repeats runs after one warm-up.

    python tools/light_probes_timing.py [--mesh-n 1900] [--many 4096x256] [--few 64x16384] [--grid 32x32x32x64] [--lookup 1048576] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shape(text):
    return tuple(int(v) for v in text.lower().split("x"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--many", type=shape, default=(4096, 256), help="probes x samples of the many-probes case")
    ap.add_argument("--few", type=shape, default=(64, 16384), help="probes x samples of the many-samples case")
    ap.add_argument("--grid", type=shape, default=(32, 32, 32, 64), help="nx x ny x nz x samples of the grid case")
    ap.add_argument("--lookup", type=int, default=1 << 20, help="points of the lookup case")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cpupathtrace_amd import binding, scenes

    if binding.device_count() < 1:
        raise SystemExit("light_probes_timing needs a GPU")
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

    pos, nrm = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
    cases = [("DragonBox, %d triangles" % len(pos), scenes.dragon_box_scene(pos, nrm, aspect_ratio=-1.0)), ("Box", scenes.box_scene(aspect_ratio=-1.0))]
    say("light_probes_timing: device %s; median of %d runs" % (torch.cuda.get_device_name(0), args.repeats))
    for name, (sc, _) in cases:
        gpu = binding.Scene(sc, device=0)
        try:
            eps = 1e-3
            rng = np.random.default_rng(0)
            # gather points: what random rays from a place inside the scene hit, the normals turned against them (tools/gather_probe.py)
            d = rng.normal(size=(1 << 16, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            rays = np.concatenate([np.tile(np.array([0.5, 0.5, 0.5]), (len(d), 1)), d], axis=1).astype(np.float32)
            hit = gpu.query(rays)
            rays, hit = rays[hit["object"] >= 0], hit[hit["object"] >= 0]
            normal = np.where(((hit["normal"] * rays[:, 3:]).sum(axis=1) > 0)[:, None], -hit["normal"], hit["normal"])
            surface = np.ascontiguousarray(np.concatenate([hit["position"], normal], axis=1), np.float32)
            say("%s" % name)
            say("  %-22s %10s %8s %10s %14s %12s %14s   %s" % ("case", "probes", "samples", "ms", "Msamples/s", "gather ms", "gather Ms/s", "mean band 0, missed, backfacing"))

            def probes_case(label, n, samples, positions):
                d_out = torch.empty((n, 32), dtype=torch.int32, device="cuda:0")
                d_pos = torch.from_numpy(positions).to("cuda:0")
                call = lambda: gpu.light_probes_device(d_pos.data_ptr(), n, d_out.data_ptr(), samples, eps, 1, stream.cuda_stream)
                pts = np.ascontiguousarray(np.resize(surface, (n, 6)))
                d_pts = torch.from_numpy(pts).to("cuda:0")
                d_g = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
                gather_ms = device(lambda: gpu.gather_device(d_pts.data_ptr(), n, d_g.data_ptr(), binding.GATHER_PATHS, samples, eps, np.inf, 1, stream.cuda_stream))
                ms = device(call)
                got = d_out.cpu().numpy().view(binding.LightProbe).ravel()
                say("  %-22s %10d %8d %10.2f %14.1f %12.2f %14.1f   %s, %.3f, %.3f" % (label, n, samples, ms, n * samples / ms / 1e3, gather_ms, n * samples / gather_ms / 1e3,
                    np.array2string(np.nanmean(got["sh"][:, 0], axis=0), precision=4), got["missed"].sum() / (n * samples), got["backfacing"].sum() / (n * samples)))
                return ms

            for label, (n, samples) in (("many probes", args.many), ("many samples", args.few)):
                positions = np.ascontiguousarray(rng.uniform(-0.8, 0.8, (n, 3)), np.float32)
                probes_case(label, n, samples, positions)
            # the grid's nodes, made on the host here so that the device form can be timed with events (pt_light_probes_grid has a host
            # form only): the same positions and records as it makes on the device
            nx, ny, nz, samples = args.grid
            origin, step = (-0.9, -0.9, -0.9), (1.8 / max(nx - 1, 1), 1.8 / max(ny - 1, 1), 1.8 / max(nz - 1, 1))
            grid = binding.light_probe_grid(origin, step, (nx, ny, nz))
            iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
            idx = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1).astype(np.float32)
            nodes = np.ascontiguousarray(grid["origin"] + idx * grid["step"], np.float32)
            probes_case("grid %dx%dx%d" % (nx, ny, nz), len(nodes), samples, nodes)
            # a bound on the projection's share: probes far outside, whose samples all miss at the root box
            n, samples = args.many
            far = np.ascontiguousarray(rng.uniform(50.0, 60.0, (n, 3)), np.float32)
            d_far = torch.from_numpy(far).to("cuda:0")
            d_out = torch.empty((n, 32), dtype=torch.int32, device="cuda:0")
            miss_ms = device(lambda: gpu.light_probes_device(d_far.data_ptr(), n, d_out.data_ptr(), samples, eps, 1, stream.cuda_stream))
            d_in = torch.from_numpy(np.ascontiguousarray(rng.uniform(-0.8, 0.8, (n, 3)), np.float32)).to("cuda:0")
            inside_ms = device(lambda: gpu.light_probes_device(d_in.data_ptr(), n, d_out.data_ptr(), samples, eps, 1, stream.cuda_stream))
            say("  projection: a call whose samples all miss (sampling at its cheapest + the projection), %d x %d: %.3f ms: at most %.1f %% of the call inside the scene (%.2f ms)" % (
                n, samples, miss_ms, 100.0 * miss_ms / inside_ms, inside_ms))
            # the lookup
            m = args.lookup
            _, records = gpu.light_probe_grid(origin, step, (nx, ny, nz), samples=4, epsilon=eps, base_seed=1)
            d_rec = torch.from_numpy(records.ravel().view(np.uint8).reshape(-1, 128)).to("cuda:0")
            pts = np.concatenate([rng.uniform(-1.0, 1.0, (m, 3)), d[np.arange(m) % len(d)]], axis=1).astype(np.float32)
            d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to("cuda:0")
            d_val = torch.empty((m, 4), dtype=torch.float32, device="cuda:0")
            ms = device(lambda: gpu.shade_with_light_probes_device(grid, d_rec.data_ptr(), d_pts.data_ptr(), m, d_val.data_ptr(), 0.25, stream.cuda_stream))
            say("  lookup: %d points on the %dx%dx%d grid: %.3f ms, %.1f Mpoints/s; mean weight sum %.3f" % (m, nx, ny, nz, ms, m / ms / 1e3, float(d_val[:, 3].mean())))
        finally:
            gpu.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
