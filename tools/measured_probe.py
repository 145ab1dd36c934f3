"""What the measured preview costs next to the plain denoised one (pt_frame_get_variance, pt_frame_preview_measured).

    python tools/measured_probe.py [--workload cornell] [--sizes 256,1024] [--min-spp 16] [--max-spp 1024] [--quantum 16] [--out profiles/measured_probe.json]

A progressive frame is stopped after its first pass (every unfinished pixel rated).  Then, per size: the device time of the variance map's
gather kernel, of the plain denoised preview's filter (pt_frame_preview with the default parameters) and of the measured preview's filter
(pt_frame_preview_measured with its defaults) -- device events around the launches, read back with the diagnostic
pt_debug_frame_measured_ms; the protocol of DESIGN 4.10: one untimed call first (it allocates the buffers and renders the features), then
the median of 3."""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from cpupathtrace_amd import binding, scenes

REPEATS = 3


def measured_ms(frame):
    gather, filt = C.c_double(), C.c_double()
    binding._check(binding.load().pt_debug_frame_measured_ms(frame._h, C.byref(gather), C.byref(filt)))
    return gather.value, filt.value


def median_of(call, frame, which):
    call()
    times = []
    for _ in range(REPEATS):
        call()
        times.append(measured_ms(frame)[which])
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cornell")
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--mesh-n", type=int, default=bench.parse_args([]).mesh_n)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--quantum", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join("profiles", "measured_probe.json"))
    args = ap.parse_args()
    out = {"spp": [args.min_spp, args.max_spp], "quantum": args.quantum, "repeats": REPEATS, "frames": []}
    for size in (int(s) for s in args.sizes.split(",")):
        sc, cam, label, _ = bench.build_workload(args.workload, size, size, args.mesh_n)
        opt = scenes.options(size, size, args.min_spp, args.max_spp)
        gpu = binding.Scene(sc, device=0)
        try:
            frame = binding.Frame(gpu, cam, opt, base_seed=args.seed)
            try:
                frame.set_progressive(args.quantum, 1)
                _, _, info = frame.render()
                var = frame.variance()
                rated = int((var[..., 3] >= 2).sum())
                gather, gathers = median_of(frame.variance, frame, 0)
                plain, plains = median_of(lambda: frame.preview(denoise=True), frame, 1)
                meas, meass = median_of(frame.preview_measured, frame, 1)
                out["frames"].append({"workload": label, "frame": "%dx%d" % (size, size), "pixels_rated": rated, "pixels": size * size,
                                      "pass_kernel_ms": sum(st["kernel_ms"] for st in info["stats"]),
                                      "variance_gather_ms": gather, "variance_gather_ms_all": gathers,
                                      "plain_preview_filter_ms": plain, "plain_preview_filter_ms_all": plains,
                                      "measured_preview_filter_ms": meas, "measured_preview_filter_ms_all": meass})
            finally:
                frame.close()
        finally:
            gpu.close()
    text = json.dumps(out, indent=1, default=float)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
