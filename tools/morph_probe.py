"""Blend shapes on the device against what they took before, on the stand-in mesh of the benchmark scene: one instance
of the bumpy sphere (--mesh-n 1900: 3.6 M vertices, 7.2 M faces) in the box, a --bones-bone K = --influences rig, --sparse sparse targets
that each list about --coverage of the vertices, and one dense target.  All routes run in ONE process, alternating, after a warm-up;
every figure is the median of --repeat (5 at least) runs.

    python tools/morph_probe.py [--mesh-n 1900] [--bones 64] [--influences 4] [--sparse 50] [--coverage 0.05] [--repeat 5]

    morph               pt_scene_morph without bones: the set weighted on the device, then what a pose does
    morph + bones       pt_scene_morph with bones: the same launch carries the morphed vertices through the rig
    host + vertices     the route before: the morph evaluated in NumPy (float32, target after target), then pt_scene_deform with
                        PT_DEFORM_VERTICES; the NumPy time is reported beside the call's
    pose                a plain pt_scene_pose of the same scene: the floor
    morph kernel        the kernel's device time and its achieved bytes/s from the derived 12 + 4 + 16 * entries + 8 K + 12 bytes per
                        vertex, without and with bones, and in the cache form (PT_MORPH_LDS_TARGETS=0)

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from deform_probe import bones, description, medians, rig, timed  # noqa: E402

F = np.float32
COPY_BANDWIDTH = 6.29e12  # bytes/s, the copy bandwidth DESIGN.md records for this device


def targets(verts, n_sparse, coverage, seed=2):
    """n_sparse sparse targets -- each a patch of consecutive vertices (a region of the mesh, as a face's targets are) that covers about
    `coverage` of them -- and one dense target, a breathing of the whole shape."""
    rng = np.random.default_rng(seed)
    n = len(verts)
    out = []
    for _ in range(n_sparse):
        length = max(int(n * coverage * rng.uniform(0.8, 1.2)), 1)
        start = int(rng.integers(0, max(n - length, 1)))
        idx = np.arange(start, min(start + length, n), dtype=np.uint32)
        out.append((idx, rng.uniform(-0.5, 0.5, (len(idx), 3)).astype(F)))
    out.append((None, (0.02 * (verts - verts.mean(axis=0))).astype(F)))
    return out


def host_morph(verts, target_list, weights):
    """float32 on the host, target after target: the probe's stand-in for a user's CPU morph."""
    m = np.array(verts, F)
    for (idx, d), w in zip(target_list, weights):
        if idx is None:
            m += F(w) * d
        else:
            m[idx] += F(w) * d
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--bones", type=int, default=64)
    ap.add_argument("--influences", type=int, default=4)
    ap.add_argument("--sparse", type=int, default=50)
    ap.add_argument("--coverage", type=float, default=0.05)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    from cpupathtrace_amd import binding, scenes
    repeat = max(args.repeat, 5)
    verts, faces = scenes.bumpy_sphere_vertices(args.mesh_n, args.mesh_n)
    verts = np.ascontiguousarray(verts, F)
    matrix = np.array(scenes.DRAGON_BOX_TRANSFORM, F)
    k = args.influences
    bone, weight = rig(verts, args.bones, k)
    target_list = targets(verts, args.sparse, args.coverage)
    n_entries = sum(len(d) for _, d in target_list)
    rng = np.random.default_rng(3)
    weights = [rng.uniform(0.0, 1.0, len(target_list)).astype(F) for _ in range(repeat + 2)]
    tables = [bones(args.bones, p) for p in range(repeat + 2)]
    result = {"vertices": int(len(verts)), "faces": int(len(faces)), "bones": args.bones, "influences": k, "targets": len(target_list), "entries": int(n_entries),
              "entries_per_vertex": n_entries / len(verts), "repeat": repeat}

    live = binding.Scene(description(scenes, verts, faces, matrix))
    t0 = time.perf_counter()
    live.bind_morphs(0, target_list)
    result["bind_morphs_ms"] = 1e3 * (time.perf_counter() - t0)
    live.bind_skin(0, bone, weight, n_bones=args.bones)
    live.morph(weights={0: weights[0]})  # warm-up: buffers and scratch are grown here
    live.morph(weights={0: weights[0]}, bones={0: tables[0]})
    live.deform(vertices={0: host_morph(verts, target_list, weights[0])})
    live.pose([matrix])
    alone, fused, by_vertices, posed, host = [], [], [], [], []
    for p in range(1, repeat + 1):
        alone.append(timed(lambda: live.morph(weights={0: weights[p]})))
        fused.append(timed(lambda: live.morph(weights={0: weights[p]}, bones={0: tables[p]})))
        t0 = time.perf_counter()
        shape = host_morph(verts, target_list, weights[p])
        host.append(1e3 * (time.perf_counter() - t0))
        by_vertices.append(timed(lambda: live.deform(vertices={0: shape})))
        posed.append(timed(lambda: live.pose([matrix])))
    result["morph"], result["morph_bones"] = medians(alone), medians(fused)
    result["vertices_deform"], result["pose"] = medians(by_vertices), medians(posed)
    result["host_morph_float32_numpy_ms"] = statistics.median(host)
    result["host_route_ms"] = result["host_morph_float32_numpy_ms"] + result["vertices_deform"]["wall_ms"]
    result["allocations_first_last"] = [alone[0]["allocations"], fused[-1]["allocations"]]

    # the kernel alone: device time between two events around its launch, bytes from the derivation
    kernel = {}
    for name, kk, lds in (("morph", 0, None), ("morph_bones", k, None), ("morph_cache", 0, 0), ("morph_bones_cache", k, 0)):
        if lds is not None:
            os.environ["PT_MORPH_LDS_TARGETS"] = str(lds)
        call = (lambda: live.morph(weights={0: weights[1]}, bones={0: tables[1]})) if kk else (lambda: live.morph(weights={0: weights[1]}))
        call()
        ms = statistics.median(call()["morph_ms"] for _ in range(repeat))
        os.environ.pop("PT_MORPH_LDS_TARGETS", None)
        moved = len(verts) * (12 + 4 + 8 * kk + 12) + 16 * n_entries + 4 * len(target_list) + 48 * (args.bones if kk else 0)
        kernel[name] = {"influences": kk, "morph_ms": ms, "bytes": moved, "bytes_per_s": moved / (ms * 1e-3), "fraction_of_copy_bandwidth": moved / (ms * 1e-3) / COPY_BANDWIDTH}
    live.close()
    result["morph_kernel"] = kernel
    result["ratio_host_route_over_morph_bones"] = result["host_route_ms"] / result["morph_bones"]["wall_ms"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
