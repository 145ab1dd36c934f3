"""Cost of temporal denoising on the device: one push of pt_temporal_denoise_device (default parameters, the camera moved
since the last push so that every pixel is reprojected) next to pt_denoise_device of the same frame, at 256^2, 1024^2 and 2048^2 on the Box,
the Cornell box and the DragonBox with the procedural stand-in mesh, each the median of three runs timed with device events.

    python tools/temporal_probe.py [--sizes 256,1024,2048] [--mesh-n 300] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# per pixel, what the accumulate step moves at least once (pt_denoise.hip): features 48, prepared colour 16, class 4 in; the 4 taps' history
# (class 4, normal 16, position 16, colour 16, moments 8, length 4) = 4 x 64, served by the caches for neighbouring pixels, so about one
# tap's 64 from HBM; out: colour 16, moments 8, length 4, position 16, normal 16
ACCUMULATE_BYTES = 48 + 16 + 4 + 64 + 16 + 8 + 4 + 16 + 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,2048")
    ap.add_argument("--mesh-n", type=int, default=300, help="stand-in mesh resolution (300 -> 179,400 triangles)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from cpupathtrace_amd import binding, scenes

    if binding.device_count() < 1:
        raise SystemExit("temporal_probe needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sizes = [int(s) for s in args.sizes.split(",")]
    mesh = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
    cases = [("box", lambda w: scenes.box_scene()), ("cornell", lambda w: scenes.cornell_scene(w, w)),
             ("dragon_standin_%dtri" % len(mesh[0]), lambda w: scenes.dragon_box_scene(*mesh))]
    say("temporal_probe: device %s; median of %d runs, device events; default parameters %s" % (
        torch.cuda.get_device_name(0), args.repeats, binding.temporal_params_default()))
    say("%-28s %6s %12s %12s %8s %14s" % ("scene", "size", "denoise ms", "temporal ms", "ratio", "Mpix/s (tmp)"))
    stream = torch.cuda.current_stream()
    for name, make in cases:
        for w in sizes:
            sc, cam = make(w)
            moved = dict(cam, origin=(cam["origin"][0] + 0.01, cam["origin"][1], cam["origin"][2]))
            gpu = binding.Scene(sc, device=0)
            t = binding.TemporalDenoiser(w, w)
            try:
                opt = scenes.options(w, w, 1, 1)
                img = torch.rand((w, w, 4), dtype=torch.float32, device="cuda:0")
                feat = torch.empty((w, w, 3, 4), dtype=torch.float32, device="cuda:0")
                feat2 = torch.empty_like(feat)
                out = torch.empty_like(img)
                hist = torch.empty((w, w), dtype=torch.int32, device="cuda:0")
                gpu.render_features_device(cam, opt, feat.data_ptr(), stream.cuda_stream)
                gpu.render_features_device(moved, opt, feat2.data_ptr(), stream.cuda_stream)
                t_dn, t_tp = [], []
                for rep in range(args.repeats + 1):  # the first round warms up
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    t.denoise_device(img.data_ptr(), feat.data_ptr(), cam, out.data_ptr(), hist.data_ptr(), stream.cuda_stream)
                    e[0].record(stream)
                    binding.denoise_device(img.data_ptr(), feat2.data_ptr(), w, w, out.data_ptr(), stream.cuda_stream)
                    e[1].record(stream)
                    t.denoise_device(img.data_ptr(), feat2.data_ptr(), moved, out.data_ptr(), hist.data_ptr(), stream.cuda_stream)
                    e[2].record(stream)
                    torch.cuda.synchronize()
                    if rep > 0:
                        t_dn.append(e[0].elapsed_time(e[1]))
                        t_tp.append(e[1].elapsed_time(e[2]))
                d, tp = statistics.median(t_dn), statistics.median(t_tp)
                say("%-28s %6d %12.3f %12.3f %8.2f %14.1f" % (name, w, d, tp, tp / d, w * w / tp / 1e3))
            finally:
                t.close()
                gpu.close()
    say("the accumulate step moves at least %d B/pixel (from shapes): at 1024^2 %.1f MB -> %.4f ms at 6.29 TB/s measured" % (
        ACCUMULATE_BYTES, ACCUMULATE_BYTES * 1024 * 1024 / 1e6, ACCUMULATE_BYTES * 1024 * 1024 / 6.29e12 * 1e3))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
