"""Cost of the followed feature pass against the first-hit pass: pt_render_features_device and
pt_render_features_followed_device (max_bounces 8, and 0: the loop's own overhead) at 256^2 and 1024^2 on the Box (no specular surface),
the Cornell box and the DragonBox with the procedural stand-in mesh.  Device events, one untimed call, then the median of three.

--first-only measures the first-hit pass alone: run with PT_LIB_OVERRIDE pointing at another build of the library (the parent commit's,
which has no followed entry points) for the comparison across builds.

    python tools/follow_probe.py [--sizes 256,1024] [--mesh-n 300] [--first-only] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--mesh-n", type=int, default=300, help="stand-in mesh resolution (300 -> 179,400 triangles)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--first-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from cpupathtrace_amd import binding, scenes

    if binding.device_count() < 1:
        raise SystemExit("follow_probe needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sizes = [int(s) for s in args.sizes.split(",")]
    mesh = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
    cases = [("box", lambda w: scenes.box_scene()), ("cornell", lambda w: scenes.cornell_scene(w, w)),
             ("dragon_standin_%dtri" % len(mesh[0]), lambda w: scenes.dragon_box_scene(*mesh))]
    passes = [("first-hit", None)] if args.first_only else [("first-hit", None), ("followed 0", {"max_bounces": 0}), ("followed 8", {"max_bounces": 8})]
    say("follow_probe: device %s; library %s; one untimed call, then the median of %d, device events (min..max in brackets)" % (
        torch.cuda.get_device_name(0), os.path.basename(os.path.dirname(binding.LIB_PATH)) + "/" + os.path.basename(binding.LIB_PATH), args.repeats))
    say("%-28s %6s " % ("scene", "size") + " ".join("%-30s" % (name + " ms") for name, _ in passes))
    stream = torch.cuda.current_stream()
    for name, make in cases:
        for w in sizes:
            sc, cam = make(w)
            gpu = binding.Scene(sc, device=0)
            try:
                opt = scenes.options(w, w, 1, 1)
                feat = torch.empty((w, w, 3, 4), dtype=torch.float32, device="cuda:0")
                cells = []
                for _, followed in passes:
                    times = []
                    for rep in range(args.repeats + 1):  # the first call is not timed
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        if followed is None:
                            gpu.render_features_device(cam, opt, feat.data_ptr(), stream.cuda_stream)
                        else:
                            gpu.render_features_device(cam, opt, feat.data_ptr(), stream.cuda_stream, followed=followed)
                        e1.record(stream)
                        torch.cuda.synchronize()
                        if rep > 0:
                            times.append(e0.elapsed_time(e1))
                    cells.append("%8.3f [%7.3f..%7.3f]    " % (statistics.median(times), min(times), max(times)))
                say("%-28s %6d " % (name, w) + " ".join(cells))
            finally:
                gpu.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
