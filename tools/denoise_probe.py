"""Cost of feature-guided denoising on the device: the feature pass (pt_render_features_device) and the denoiser
(pt_denoise_device, default parameters) at 256^2, 1024^2 and 2048^2 on the Box, the Cornell box and the DragonBox with the procedural
stand-in mesh, each the median of three runs timed with device events; and the bytes an a-trous pass must move, computed from shapes,
against the HBM bandwidth of the MI355X (MI355X_MICROARCH.md: 8.0 TB/s peak, 6.29 TB/s measured float4 copy).

    python tools/denoise_probe.py [--sizes 256,1024,2048] [--mesh-n 300] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, HBM_MEASURED = 8.0e12, 6.29e12

# per pixel and pass, what the a-trous kernel must read and write at least once (pt_denoise.hip): colour + luminance in (16 B), variance
# in (4), guide (16), class (4), depth gradient (8); colour out (16), variance out (4).  Each tap beyond the pixel's own is served by the
# caches when the pass runs as planned: 24 neighbours x (class 4 + guide 16 + colour 16 + variance 4) + 8 prefilter variances x 4.
PASS_BYTES = 16 + 4 + 16 + 4 + 8 + 16 + 4
PASS_TAP_BYTES = 24 * (4 + 16 + 16 + 4) + 8 * 4


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
        raise SystemExit("denoise_probe needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sizes = [int(s) for s in args.sizes.split(",")]
    mesh = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
    cases = [("box", lambda w: scenes.box_scene()), ("cornell", lambda w: scenes.cornell_scene(w, w)),
             ("dragon_standin_%dtri" % len(mesh[0]), lambda w: scenes.dragon_box_scene(*mesh))]
    say("denoise_probe: device %s; median of %d runs, device events; denoiser: default parameters %s" % (
        torch.cuda.get_device_name(0), args.repeats, binding.denoise_params_default()))
    say("%-28s %6s %12s %12s %14s %12s" % ("scene", "size", "features ms", "denoise ms", "ms per pass*", "Mpix/s (dn)"))
    stream = torch.cuda.current_stream()
    for name, make in cases:
        for w in sizes:
            sc, cam = make(w)
            gpu = binding.Scene(sc, device=0)
            try:
                opt = scenes.options(w, w, 1, 1)
                img = torch.rand((w, w, 4), dtype=torch.float32, device="cuda:0")
                feat = torch.empty((w, w, 3, 4), dtype=torch.float32, device="cuda:0")
                out = torch.empty_like(img)
                t_feat, t_dn, t_dn1 = [], [], []
                for rep in range(args.repeats + 1):  # the first round warms up
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                    e[0].record(stream)
                    gpu.render_features_device(cam, opt, feat.data_ptr(), stream.cuda_stream)
                    e[1].record(stream)
                    binding.denoise_device(img.data_ptr(), feat.data_ptr(), w, w, out.data_ptr(), stream.cuda_stream)
                    e[2].record(stream)
                    binding.denoise_device(img.data_ptr(), feat.data_ptr(), w, w, out.data_ptr(), stream.cuda_stream, params={"iterations": 0})
                    e[3].record(stream)
                    torch.cuda.synchronize()
                    if rep > 0:
                        t_feat.append(e[0].elapsed_time(e[1]))
                        t_dn.append(e[1].elapsed_time(e[2]))
                        t_dn1.append(e[2].elapsed_time(e[3]))
                f, d, d0 = statistics.median(t_feat), statistics.median(t_dn), statistics.median(t_dn1)
                per_pass = (d - d0) / 5.0
                say("%-28s %6d %12.3f %12.3f %14.4f %12.1f" % (name, w, f, d, per_pass, w * w / d / 1e3))
            finally:
                gpu.close()
    say("* (denoise ms - denoise ms with 0 passes) / 5: the a-trous pass alone; the 0-pass call is prepare + variance + finish")
    say("bytes per a-trous pass, from shapes: %d B/pixel compulsory (in: colour 16, variance 4, guide 16, class 4, gradient 8; out: colour 16, "
        "variance 4) + %d B/pixel of neighbour taps served by L1/L2 when the pass runs as planned" % (PASS_BYTES, PASS_TAP_BYTES))
    for w in sizes:
        b = PASS_BYTES * w * w
        say("  %5d^2: %.1f MB compulsory -> %.4f ms at 6.29 TB/s measured, %.4f ms at 8.0 TB/s peak; with every tap from HBM: %.3f ms at 6.29 TB/s" % (
            w, b / 1e6, b / HBM_MEASURED * 1e3, b / HBM_PEAK * 1e3, (b + PASS_TAP_BYTES * w * w) / HBM_MEASURED * 1e3))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
