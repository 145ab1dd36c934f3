"""What a noise target costs and saves on a progressive frame (pt_frame_get_noise, pt_frame_set_noise_target).

    python tools/noise_probe.py [--workload dragon] [--size 1024] [--min-spp 16] [--max-spp 256] [--quantum 16] [--target T] [--out profiles/noise_probe.json]

1. The price of rating: after two passes the frame is rated; the device time of the rating kernel (events around it, read back with the
   diagnostic pt_debug_frame_noise_ms) next to the kernel time of the pass before it.
2. The samples a target saves: one frame renders with the target (every pixel at or below it is held) until the target is reached on the
   whole frame; another renders even passes, every unfinished pixel a quantum per pass, until its largest error is at or below the same
   target.  Both then have no unfinished pixel above the target; the samples each drew are compared.  Without --target, the target is half
   the median error after the first two passes."""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from cpupathtrace_amd import binding, scenes

MAX_CALLS = 1000


def one_pass(frame):
    _, _, info = frame.render()
    return info, sum(st["samples"] for st in info["stats"]), sum(st["kernel_ms"] for st in info["stats"])


def rate_ms(frame):
    ms = C.c_double()
    binding._check(binding.load().pt_debug_frame_noise_ms(frame._h, C.byref(ms)))
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="dragon")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--mesh-n", type=int, default=bench.parse_args([]).mesh_n)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=256)
    ap.add_argument("--quantum", type=int, default=16)
    ap.add_argument("--target", type=float, default=0.0)
    ap.add_argument("--floor", type=float, default=1e-5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join("profiles", "noise_probe.json"))
    args = ap.parse_args()
    sc, cam, label, _ = bench.build_workload(args.workload, args.size, args.size, args.mesh_n)
    opt = scenes.options(args.size, args.size, args.min_spp, args.max_spp)
    gpu = binding.Scene(sc, device=0)
    out = {"workload": label, "frame": "%dx%d" % (args.size, args.size), "spp": [args.min_spp, args.max_spp], "quantum": args.quantum, "floor": args.floor}
    try:
        held, even = binding.Frame(gpu, cam, opt, base_seed=args.seed), binding.Frame(gpu, cam, opt, base_seed=args.seed)
        try:
            drawn = {"held": 0, "even": 0}
            passes = {"held": 0, "even": 0}
            for name, frame in (("held", held), ("even", even)):
                frame.set_progressive(args.quantum, 1)
                for _ in range(2):
                    info, samples, kernel_ms = one_pass(frame)
                    drawn[name] += samples
                    passes[name] += 1
            held.noise()  # (the first call allocates its buffers)
            noise = held.noise()
            out["rating"] = {"streams_rated": noise["streams_rated"], "rate_kernel_ms": rate_ms(held), "pass_kernel_ms": kernel_ms,
                             "pass_samples": samples, "max_error": noise["max_error"], "median_error_upper_bound": noise.percentile(50)}
            target = args.target or float(np.median(held.error_map()[held.error_map() > 0])) / 2
            out["target"] = target
            held.set_noise_target(target, args.floor, 1.0)
            while not held.done and not held.noise()["target_reached"]:
                assert passes["held"] < MAX_CALLS
                info, samples, _ = one_pass(held)
                drawn["held"] += samples
                passes["held"] += 1
            while not even.done and even.noise()["max_error"] > target:
                assert passes["even"] < MAX_CALLS
                info, samples, _ = one_pass(even)
                drawn["even"] += samples
                passes["even"] += 1
            for name, frame in (("held", held), ("even", even)):
                n = frame.noise()
                out[name] = {"samples": drawn[name], "passes": passes[name], "streams_finished": n["streams_finished"], "streams_held": n["streams_held"],
                             "max_error": n["max_error"], "complete": bool(frame.done)}
            out["samples_saved_fraction"] = 1.0 - drawn["held"] / float(drawn["even"])
        finally:
            held.close()
            even.close()
    finally:
        gpu.close()
    text = json.dumps(out, indent=1, default=float)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
