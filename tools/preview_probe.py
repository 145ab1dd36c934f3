"""Cost and coverage of the preview of an unfinished frame (pt_frame_preview) on the Box and the DragonBox with the
procedural stand-in mesh, at 1024^2 and 1920x1080 (1024 spp, the metric frame's count):
  - the fraction of pixels that have samples (finished or parked) after the frame's first 100 ms slice;
  - the raw and the denoised preview, each the median of three calls, timed on the host around the call (it synchronises its stream
    before it returns); the first denoised preview also runs the feature pass, reported as the difference to the later ones;
  - the host<->device copies a preview makes of the image (16 B/pixel each way, plus 4 B/pixel of sample counts back), the same sizes
    from and to pageable numpy memory, timed with device events (median of three), to see whether they dominate the raw preview.
The kernels alone: run this under rocprofv3 --kernel-trace --stats (pt_frame_gather_kernel, pt_frame_preview_base_kernel,
pt_frame_scatter_kernel, the masked pt_denoise_* instantiations).

    python tools/preview_probe.py [--mesh-n 1900] [--progressive Q] [--cases box,dragon] [--out FILE]
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
    ap.add_argument("--mesh-n", type=int, default=1900, help="stand-in mesh resolution (1900 -> 7.2 M triangles, bench.py's default)")
    ap.add_argument("--slice-ms", type=float, default=100.0)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--progressive", type=int, default=0, metavar="Q",
                    help="render the first slice as one progressive pass of Q samples per pixel instead of a budgeted slice (DESIGN.md 4.14)")
    ap.add_argument("--cases", default="box,dragon", help="comma-separated: box, dragon")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cpupathtrace_amd import binding, scenes

    if binding.device_count() < 1:
        raise SystemExit("preview_probe needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def med(f):
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    def copy_ms(w, h):
        """H2D of the image from pageable memory, D2H of the image and of the sample counts to pageable memory; device events."""
        host = np.zeros((h, w, 4), np.float32)
        host_s = np.zeros((h, w), np.int32)
        dev = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        dev_s = torch.empty((h, w), dtype=torch.int32, device="cuda:0")
        up, down = [], []
        for rep in range(args.repeats + 1):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            dev.copy_(torch.from_numpy(host))
            e[1].record()
            torch.from_numpy(host).copy_(dev)
            torch.from_numpy(host_s).copy_(dev_s)
            e[2].record()
            torch.cuda.synchronize()
            if rep > 0:
                up.append(e[0].elapsed_time(e[1]))
                down.append(e[1].elapsed_time(e[2]))
        return statistics.median(up), statistics.median(down)

    cases = []
    if "box" in args.cases.split(","):
        cases.append(("box", lambda a: scenes.box_scene(aspect_ratio=a)))
    if "dragon" in args.cases.split(","):
        mesh = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
        cases.append(("dragon_standin_%dtri" % len(mesh[0]), lambda a: scenes.dragon_box_scene(*mesh, aspect_ratio=a)))
    sizes = [(1024, 1024), (1920, 1080)]
    first_slice = "one progressive pass of %d samples" % args.progressive if args.progressive > 0 else "%.0f ms" % args.slice_ms
    say("preview_probe: device %s; %d spp; first slice %s; preview times: median of %d calls, host clock around the call" % (
        torch.cuda.get_device_name(0), args.spp, first_slice, args.repeats))
    say("%-30s %10s %9s %9s %9s %9s %10s %10s %10s" % ("scene", "size", "covered", "parked", "untouched", "raw ms", "denoise ms",
                                                       "1st dn ms", "features*"))
    for name, make in cases:
        for w, h in sizes:
            sc, cam = make(-float(w) / float(h))
            gpu = binding.Scene(sc, device=0)
            try:
                opt = scenes.options(w, h, args.spp, args.spp)
                frame = binding.Frame(gpu, cam, opt, base_seed=1234)
                try:
                    if args.progressive > 0:
                        frame.set_progressive(args.progressive, 1)
                        frame.render()
                    else:
                        frame.render(budget_ms=args.slice_ms)
                    _, samples = frame.preview()
                    fi = frame.info()
                    covered = float((samples != 0).mean())
                    raw = med(lambda: frame.preview())
                    t0 = time.perf_counter()
                    frame.preview(denoise=True)  # (the feature pass runs here, once per frame)
                    first = (time.perf_counter() - t0) * 1e3
                    dn = med(lambda: frame.preview(denoise=True))
                    say("%-30s %10s %9.4f %9d %9d %9.2f %10.2f %10.2f %10.2f" % (name, "%dx%d" % (w, h), covered, fi["streams_parked"],
                                                                                 fi["streams_untouched"], raw, dn, first, first - dn))
                finally:
                    frame.close()
            finally:
                gpu.close()
    say("covered: pixels with samples (finished or parked) after the first slice; * first denoised preview minus the median of the later ones")
    for w, h in sizes:
        up, down = copy_ms(w, h)
        say("copies at %dx%d: image H2D %.2f ms (%.1f MB from pageable memory), image + samples D2H %.2f ms (%.1f MB); device events" % (
            w, h, up, w * h * 16 / 1e6, down, w * h * 20 / 1e6))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
