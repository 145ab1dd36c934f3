"""Cost of motion for deformed meshes on the device: pt_render_features_motion_marked_device, with the one instance
DEFORMED, next to pt_render_features_motion_device on the same frame (whose kernel this feature leaves untouched), and the wall time of a
mark, at 256^2, 1024^2 and 2048^2 on the Cornell box with one bumpy-sphere instance whose vertices are replaced between mark and frame;
feature passes are the median of three runs timed with device events.

    python tools/motion_shapes_probe.py [--sizes 256,1024,2048] [--out FILE]
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
    ap.add_argument("--sizes", default="256,1024,2048")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cpupathtrace_amd import binding, scenes

    if binding.device_count() < 1:
        raise SystemExit("motion_shapes_probe needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    vertices, faces = scenes.bumpy_sphere_vertices(48, 24)
    here = np.array(scenes.DRAGON_BOX_TRANSFORM, np.float32)
    here[:3, :3] *= np.float32(0.6)
    here[:3, 3] += np.array([0.0, -0.3, -0.3], np.float32)
    before = here.copy()
    before[:3, 3] += np.array([-0.05, 0.0, 0.02], np.float32)  # (the matrix route's previous pose: its instance is MOVED)
    bent = vertices.copy()
    bent[:, 0] += np.float32(0.002) * (vertices[:, 1] - 50.0) ** 2  # the sphere (radius 40 around (0, 50, 0)) leans over
    say("motion_shapes_probe: device %s; median of %d runs, device events; Cornell box + one instance of %d faces, deformed after the mark" % (
        torch.cuda.get_device_name(0), args.repeats, len(faces)))
    say("%6s %14s %14s %8s %10s %12s" % ("size", "by matrices ms", "marked ms", "ratio", "mark ms", "deformed px"))
    stream = torch.cuda.current_stream()
    for w in [int(s) for s in args.sizes.split(",")]:
        sc, cam = scenes.cornell_scene(w, w)
        sc = dict(sc, meshes=[(vertices, faces)], instances=[{"mesh": 0, "transform": here, "smooth": True, "cull": True, "material": scenes.NO_MATERIAL}])
        gpu = binding.Scene(sc, device=0)
        try:
            opt = scenes.options(w, w, 1, 1)
            feat = torch.empty((w, w, 3, 4), dtype=torch.float32, device="cuda:0")
            motion = torch.empty((w, w, 2, 4), dtype=torch.float32, device="cuda:0")
            gpu.deform(vertices={0: vertices})  # (the mesh has current vertices: the mark copies them)
            marks = []
            for _ in range(args.repeats + 1):
                t0 = time.perf_counter()
                gpu.mark_motion()
                marks.append((time.perf_counter() - t0) * 1e3)
            gpu.deform(vertices={0: bent})
            assert gpu.motion_mark()[1].tolist() == [binding.MOTION_DEFORMED]
            t_m, t_s = [], []
            for rep in range(args.repeats + 1):  # the first round warms up
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record(stream)
                gpu.render_features_motion_device(cam, opt, feat.data_ptr(), motion.data_ptr(), stream.cuda_stream, previous=[before])
                e[1].record(stream)
                gpu.render_features_motion_marked_device(cam, opt, feat.data_ptr(), motion.data_ptr(), stream.cuda_stream)
                e[2].record(stream)
                torch.cuda.synchronize()
                if rep > 0:
                    t_m.append(e[0].elapsed_time(e[1]))
                    t_s.append(e[1].elapsed_time(e[2]))
            m, s = statistics.median(t_m), statistics.median(t_s)
            on = float((motion[..., 0, 3] > 0).float().mean())
            say("%6d %14.3f %14.3f %8.2f %10.3f %11.1f %%" % (w, m, s, s / m, statistics.median(marks[1:]), 100 * on))
        finally:
            gpu.close()
    say("a mark of this scene copies %d B of vertices device to device; the marked pass reads per hit ray on a deformed instance 4 B of the face table, 12 B of indices, 36 B "
        "of vertices and a 192 B table entry more than the matrix route" % (12 * len(vertices)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
