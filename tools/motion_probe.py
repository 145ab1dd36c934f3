"""Cost of motion-aware temporal denoising on the device: pt_render_features_motion_device next to
pt_render_features_device (whose kernel this feature leaves untouched) on the same scene and camera, and one motion push of
pt_temporal_denoise_motion_device next to a plain push of the same frame, at 256^2, 1024^2 and 2048^2 on the Cornell box with one posed
bumpy-sphere instance, each the median of three runs timed with device events.

    python tools/motion_probe.py [--sizes 256,1024,2048] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MOTION_BYTES = 32  # per pixel: what the feature pass writes more, and what the push reads more (2 float4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,2048")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cpupathtrace_amd import binding, scenes

    if binding.device_count() < 1:
        raise SystemExit("motion_probe needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    vertices, faces = scenes.bumpy_sphere_vertices(48, 24)
    here = np.array(scenes.DRAGON_BOX_TRANSFORM, np.float32)
    here[:3, :3] *= np.float32(0.6)
    here[:3, 3] += np.array([0.0, -0.3, -0.3], np.float32)
    before = here.copy()
    before[:3, 3] += np.array([-0.05, 0.0, 0.02], np.float32)
    say("motion_probe: device %s; median of %d runs, device events; Cornell box + one instance of %d faces" % (
        torch.cuda.get_device_name(0), args.repeats, len(faces)))
    say("%6s %12s %12s %8s %12s %12s %8s" % ("size", "features ms", "+motion ms", "ratio", "push ms", "motion push", "ratio"))
    stream = torch.cuda.current_stream()
    for w in [int(s) for s in args.sizes.split(",")]:
        sc, cam = scenes.cornell_scene(w, w)
        sc = dict(sc, meshes=[(vertices, faces)], instances=[{"mesh": 0, "transform": before, "smooth": True, "cull": True, "material": scenes.NO_MATERIAL}])
        gpu = binding.Scene(sc, device=0)
        plain, moving = binding.TemporalDenoiser(w, w), binding.TemporalDenoiser(w, w)
        try:
            opt = scenes.options(w, w, 1, 1)
            img = torch.rand((w, w, 4), dtype=torch.float32, device="cuda:0")
            feat = torch.empty((w, w, 3, 4), dtype=torch.float32, device="cuda:0")
            feat0 = torch.empty_like(feat)
            motion = torch.empty((w, w, 2, 4), dtype=torch.float32, device="cuda:0")
            out = torch.empty_like(img)
            hist = torch.empty((w, w), dtype=torch.int32, device="cuda:0")
            gpu.render_features_device(cam, opt, feat0.data_ptr(), stream.cuda_stream)
            gpu.pose([here])
            t_f, t_m, t_p, t_q = [], [], [], []
            for rep in range(args.repeats + 1):  # the first round warms up
                e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
                for t in (plain, moving):  # the history both pushes below reproject: the frame before the pose
                    t.reset()
                    t.denoise_device(img.data_ptr(), feat0.data_ptr(), cam, out.data_ptr(), hist.data_ptr(), stream.cuda_stream)
                e[0].record(stream)
                gpu.render_features_device(cam, opt, feat.data_ptr(), stream.cuda_stream)
                e[1].record(stream)
                gpu.render_features_motion_device(cam, opt, feat.data_ptr(), motion.data_ptr(), stream.cuda_stream, previous=[before])
                e[2].record(stream)
                plain.denoise_device(img.data_ptr(), feat.data_ptr(), cam, out.data_ptr(), hist.data_ptr(), stream.cuda_stream)
                e[3].record(stream)
                moving.denoise_device(img.data_ptr(), feat.data_ptr(), cam, out.data_ptr(), hist.data_ptr(), stream.cuda_stream, motion=motion.data_ptr())
                e[4].record(stream)
                torch.cuda.synchronize()
                if rep > 0:
                    t_f.append(e[0].elapsed_time(e[1]))
                    t_m.append(e[1].elapsed_time(e[2]))
                    t_p.append(e[2].elapsed_time(e[3]))
                    t_q.append(e[3].elapsed_time(e[4]))
            f, m, p, q = (statistics.median(t) for t in (t_f, t_m, t_p, t_q))
            moved = float((motion[..., 0, 3] > 0).float().mean())
            say("%6d %12.3f %12.3f %8.2f %12.3f %12.3f %8.2f   (%.1f %% of the pixels on the moved instance)" % (w, f, m, m / f, p, q, q / p, 100 * moved))
        finally:
            plain.close()
            moving.close()
            gpu.close()
    say("expected from shapes: %d B/pixel more written by the feature pass and read by the push: at 1024^2 %.1f MB -> %.4f ms at 6.29 TB/s measured" % (
        MOTION_BYTES, MOTION_BYTES * 1024 * 1024 / 1e6, MOTION_BYTES * 1024 * 1024 / 6.29e12 * 1e3))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
