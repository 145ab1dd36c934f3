"""Cost of the light-group passes on the device, on scene G of the tests (tests/gather_cases.py: two emissive materials, two
point lights, glass and mirrors) and on the benchmark scene (the DragonBox with its stand-in mesh): pt_light_passes_rays_device at
P = 1, 4, 8 and 24 passes beside pt_radiance_rays_device with the same rays, samples and seed -- the existing call is the baseline, in the
same process, and the ratio is printed beside the two times.  Material m is in group m mod n_groups, point light j in group
(materials + j) mod n_groups; P = 24 is 8 groups with the split.  Figures are device events around the call on torch's stream, the median
of --repeats runs after one warm-up.

Every (scene, P) step runs in a process of its own under its own time limit; after a step that fails or runs out of time nothing more is
started.

With --chunk the steps run with PT_RADIANCE_CHUNK set to that many pairs (the baseline's 1 Mi pairs fit one launch either way): a launch
of the passes holds PT_RADIANCE_CHUNK / P pairs, so this separates what the smaller launches cost from what the accumulators cost.

    python tools/light_passes_timing.py [--mesh-n 1900] [--rays 4096x256] [--repeats 5] [--timeout 240] [--passes 1,4,8,24] [--chunk PAIRS] [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PASSES = [1, 4, 8, 24]
SCENES = ["G", "DragonBox"]


def shape(text):
    return tuple(int(v) for v in text.lower().split("x"))


def step(args, name, n_passes):
    """One (scene, P): prints one line."""
    import numpy as np
    import torch
    from cpupathtrace_amd import binding, scenes

    if binding.device_count() < 1:
        raise SystemExit("light_passes_timing needs a GPU")
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

    rng = np.random.default_rng(0)
    n, samples = args.rays
    if name == "G":
        from tests import gather_cases
        sc, _, _ = gather_cases.build_g()
        label = "G"
        origins = rng.uniform(-0.8, 0.8, (n, 3)) + np.array([0.0, 0.0, 0.9])  # inside the room
    else:
        pos, nrm = scenes.bumpy_sphere_mesh(args.mesh_n, args.mesh_n, scenes.DRAGON_BOX_TRANSFORM)
        sc, _ = scenes.dragon_box_scene(pos, nrm, aspect_ratio=-1.0)
        label = "DragonBox, %d triangles" % len(pos)
        origins = rng.uniform(-0.8, 0.8, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n_materials, n_lights = len(sc["materials"]), len(sc["light_pos"])
    n_groups, split = (8, True) if n_passes == 24 else (n_passes, False)
    groups = binding.light_groups(n_groups, np.arange(n_materials) % n_groups, (n_materials + np.arange(n_lights)) % n_groups, split)
    assert groups.n_passes == n_passes
    gpu = binding.Scene(sc, device=0)
    try:
        eps = 1e-3
        d_rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([origins, d], axis=1), np.float32)).to("cuda:0")
        d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
        d_passes = torch.empty((n * n_passes, 4), dtype=torch.int32, device="cuda:0")
        d_total = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
        base_ms = device(lambda: gpu.radiance_device(d_rays.data_ptr(), n, d_out.data_ptr(), samples, eps, 1, stream.cuda_stream))
        ms = device(lambda: gpu.light_passes_device(d_rays.data_ptr(), n, groups, d_passes.data_ptr(), d_total.data_ptr(), samples, eps, 1, stream.cuda_stream))
        base_again = device(lambda: gpu.radiance_device(d_rays.data_ptr(), n, d_out.data_ptr(), samples, eps, 1, stream.cuda_stream))
        same = bool((d_out == d_total).all().item())
        passes = d_passes.cpu().numpy().view(binding.LightPass).reshape(n, n_passes)
        filled = int((passes["value"] != 0).any(axis=(0, 2)).sum())
        print("%-28s %d x %d, P = %2d: radiance %8.2f ms (again %8.2f), passes %8.2f ms, ratio %.3f;  %6.1f Msamples/s;  total %s, %d passes not empty" % (
            label, n, samples, n_passes, base_ms, base_again, ms, ms / base_ms, n * samples / ms / 1e3, "bit-identical" if same else "DIFFERENT", filled), flush=True)
    finally:
        gpu.close()
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--rays", type=shape, default=(4096, 256), help="rays x samples")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for one (scene, P) step")
    ap.add_argument("--passes", type=lambda t: [int(v) for v in t.split(",")], default=PASSES, help="the pass counts to time, of 1, 4, 8, 24")
    ap.add_argument("--chunk", type=int, default=None, help="PT_RADIANCE_CHUNK for the steps (default: the library's)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)  # SCENE:P -- one step, in this process
    args = ap.parse_args()
    if args.step is not None:
        name, n_passes = args.step.split(":")
        sys.exit(step(args, name, int(n_passes)))
    env = dict(os.environ)
    if args.chunk is not None:
        env["PT_RADIANCE_CHUNK"] = str(args.chunk)
    lines = ["light_passes_timing: %d rays x %d samples, median of %d runs, PT_RADIANCE_CHUNK %s" % (args.rays + (args.repeats, env.get("PT_RADIANCE_CHUNK", "default")))]
    print(lines[0], flush=True)
    status = 0
    for name in SCENES:
        for n_passes in args.passes:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%d" % (name, n_passes), "--mesh-n", str(args.mesh_n), "--rays", "%dx%d" % args.rays,
                   "--repeats", str(args.repeats)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, env=env)
            except subprocess.TimeoutExpired:
                lines.append("%s, P = %d: no answer within %d s; nothing more is started" % (name, n_passes, args.timeout))
                print(lines[-1], flush=True)
                status = 124
                break
            lines += [line for line in r.stdout.splitlines() if line]
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                lines.append("%s, P = %d: exit status %d; nothing more is started\n%s" % (name, n_passes, r.returncode, r.stderr[-2000:]))
                print(lines[-1], flush=True)
                status = r.returncode
                break
        if status != 0:
            break
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(status if status >= 0 else 1)


if __name__ == "__main__":
    main()
