"""Cost of the radiance calls on the device, on the Box scene and on the benchmark scene (the DragonBox with its stand-in
mesh): pt_radiance_rays_device for many rays x many samples beside pt_light_probes_points_device at the same pair count in the same run
-- the same loop behind another first ray, so this is the yardstick for the sampling kernel --, and an equirectangular capture beside
pt_render_tiles_device with min = max = the capture's sample count on an image of the same size -- different workloads set side by side:
the capture looks everywhere from inside the scene, the render through the scene's camera, and the render runs the persistent path
kernel.  Figures are device events around the call on torch's stream, the median of --repeats runs after one warm-up.

    python tools/radiance_timing.py [--mesh-n 1900] [--rays 4096x256] [--capture 1024x512x64] [--out FILE]
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
    ap.add_argument("--rays", type=shape, default=(4096, 256), help="rays x samples of the rays case")
    ap.add_argument("--capture", type=shape, default=(1024, 512, 64), help="width x height x samples of the capture case")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cpupathtrace_amd import binding, scenes

    if binding.device_count() < 1:
        raise SystemExit("radiance_timing needs a GPU")
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
    cases = [("Box", scenes.box_scene(aspect_ratio=-1.0)), ("DragonBox, %d triangles" % len(pos), scenes.dragon_box_scene(pos, nrm, aspect_ratio=-1.0))]
    say("radiance_timing: device %s; median of %d runs" % (torch.cuda.get_device_name(0), args.repeats))
    eps = 1e-3
    for name, (sc, cam) in cases:
        gpu = binding.Scene(sc, device=0)
        try:
            rng = np.random.default_rng(0)
            say("%s" % name)
            # rays: from places inside the scene in any direction -- what a light probe at the same place draws itself
            n, samples = args.rays
            origins = np.ascontiguousarray(rng.uniform(-0.8, 0.8, (n, 3)), np.float32)
            d = rng.normal(size=(n, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            d_rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([origins, d], axis=1), np.float32)).to("cuda:0")
            d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
            d_pos = torch.from_numpy(origins).to("cuda:0")
            d_probes = torch.empty((n, 32), dtype=torch.int32, device="cuda:0")
            probe_ms = device(lambda: gpu.light_probes_device(d_pos.data_ptr(), n, d_probes.data_ptr(), samples, eps, 1, stream.cuda_stream))
            ms = device(lambda: gpu.radiance_device(d_rays.data_ptr(), n, d_out.data_ptr(), samples, eps, 1, stream.cuda_stream))
            got = d_out.cpu().numpy().view(binding.RadianceResult).ravel()
            say("  rays     %d x %d: %8.2f ms, %7.1f Msamples/s;  light probes at the same places: %8.2f ms, %7.1f Msamples/s;  mean value %s, missed %.3f" % (
                n, samples, ms, n * samples / ms / 1e3, probe_ms, n * samples / probe_ms / 1e3, np.array2string(np.nanmean(got["value"], axis=0), precision=4),
                got["missed"].sum() / (n * samples)))
            # an equirectangular capture from the middle of the scene beside a render through the scene's camera
            width, height, spp = args.capture
            desc = binding.capture_desc(binding.CAPTURE_EQUIRECT, width, height, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0, 1, 0), jitter=True)
            d_img = torch.empty((height * width, 8), dtype=torch.int32, device="cuda:0")
            opt = scenes.options(width, height, spp, spp)
            d_frame = torch.empty((height, width, 4), dtype=torch.float32, device="cuda:0")
            render_ms = device(lambda: gpu.process_job_device(cam, opt, d_frame.data_ptr(), stream.cuda_stream, base_seed=1))
            ms = device(lambda: gpu.capture_device(desc, d_img.data_ptr(), spp, eps, 1, stream.cuda_stream))
            got = d_img.cpu().numpy().view(binding.RadianceResult).ravel()
            pairs = width * height * spp
            say("  equirect %d x %d x %d: %8.2f ms, %7.1f Msamples/s;  pt_render_tiles_device at min = max = %d: %8.2f ms, %7.1f Msamples/s;  mean value %s, missed %.3f" % (
                width, height, spp, ms, pairs / ms / 1e3, spp, render_ms, pairs / render_ms / 1e3, np.array2string(np.nanmean(got["value"], axis=0), precision=4),
                got["missed"].sum() / pairs))
        finally:
            gpu.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
