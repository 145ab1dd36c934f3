"""Deforming a mesh in place against what it took before, on the stand-in mesh of the benchmark scene: one instance of
the bumpy sphere (--mesh-n 1900: 3.6 M vertices, 7.2 M faces) in the box.  All routes run in ONE process, alternating, after a warm-up;
every figure is the median of --repeat (5 at least) runs.

    python tools/deform_probe.py [--mesh-n 1900] [--bones 64] [--influences 4] [--repeat 5]

    bones deform        pt_scene_deform with PT_DEFORM_BONES: the rig skinned on the device, then what a pose does
    vertices deform     pt_scene_deform with PT_DEFORM_VERTICES: host-skinned vertices uploaded, then what a pose does
    pose                a plain pt_scene_pose of the same scene: the floor -- a deform is a pose plus skin_ms or the upload
    destroy + create    pt_scene_destroy + pt_scene_create_meshes with the host-skinned vertices: what bending a mesh took before
                        (skinning on the host is in neither of the last three figures)
    skin kernel         the kernel's device time and its achieved bytes/s from the derived 24 + 8 K bytes per vertex, in the LDS form
                        (--bones) and in the cache form (1024 bones), for K = --influences and K = 8

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

from ingest_probe import base_builder  # noqa: E402

F = np.float32
COPY_BANDWIDTH = 6.29e12  # bytes/s, the copy bandwidth DESIGN.md records for this device


def rig(verts, n_bones, k, seed=1):
    """Bones are bands of height; a vertex follows the k bands nearest to it with weights that fall off with distance and sum to 1."""
    rng = np.random.default_rng(seed)
    y = verts[:, 1].astype(np.float64)
    band = (y - y.min()) / max(y.max() - y.min(), 1e-9) * (n_bones - 1)
    nearest = np.clip(np.round(band).astype(np.int64)[:, None] + (np.arange(k) - k // 2)[None, :], 0, n_bones - 1)
    w = 1.0 / (0.25 + np.abs(nearest - band[:, None])) * rng.uniform(0.9, 1.1, nearest.shape)
    return nearest.astype(np.uint32), (w / w.sum(axis=1, keepdims=True)).astype(F)


def bones(n_bones, phase):
    """Every band turns a little further around the vertical axis through the mesh's centre than the one below it."""
    out = np.zeros((n_bones, 3, 4), F)
    for b in range(n_bones):
        a = 0.02 * phase * b / max(n_bones - 1, 1)
        c, s = np.cos(a), np.sin(a)
        out[b] = np.array([[c, 0, s, 0], [0, 1, 0, 0.5 * phase], [-s, 0, c, 0]], F)
    return out


def host_skin(verts, bone, weight, table):
    """float64 on the host: the probe's stand-in for a user's CPU skinning (its time is reported, and is in none of the routes)."""
    homogeneous = np.concatenate([verts.astype(np.float64), np.ones((len(verts), 1))], axis=1)
    out = np.zeros((len(verts), 3))
    for k in range(bone.shape[1]):
        out += weight[:, k, None] * np.einsum("nij,nj->ni", table[bone[:, k]].astype(np.float64), homogeneous)
    return out.astype(F)


def description(scenes, verts, faces, matrix):
    sb, glass = base_builder(scenes, 1)
    sb.mesh(verts, faces, matrix, glass, cull=False, smooth=True)
    return sb.build()


def timed(call):
    t0 = time.perf_counter()
    info = call()
    return dict(info or {}, wall_ms=1e3 * (time.perf_counter() - t0))


def medians(runs):
    keys = [k for k in runs[0] if all(k in r for r in runs)]
    return {k: statistics.median(r[k] for r in runs) for k in keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--bones", type=int, default=64)
    ap.add_argument("--influences", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    from cpupathtrace_amd import binding, scenes
    repeat = max(args.repeat, 5)
    verts, faces = scenes.bumpy_sphere_vertices(args.mesh_n, args.mesh_n)
    matrix = np.array(scenes.DRAGON_BOX_TRANSFORM, F)
    k = args.influences
    bone, weight = rig(verts, args.bones, k)
    tables = [bones(args.bones, p) for p in range(repeat + 2)]
    t0 = time.perf_counter()
    shapes = [host_skin(verts, bone, weight, t) for t in tables]
    result = {"vertices": int(len(verts)), "faces": int(len(faces)), "bones": args.bones, "influences": k, "repeat": repeat,
              "host_skin_float64_numpy_ms": 1e3 * (time.perf_counter() - t0) / len(tables)}

    live = binding.Scene(description(scenes, verts, faces, matrix))
    live.bind_skin(0, bone, weight, n_bones=args.bones)
    live.deform(bones={0: tables[0]})  # warm-up: buffers and scratch are grown here
    live.deform(vertices={0: shapes[0]})
    live.pose([matrix])
    by_bones, by_vertices, posed, created = [], [], [], []
    other = None
    for p in range(1, repeat + 1):
        by_bones.append(timed(lambda: live.deform(bones={0: tables[p]})))
        by_vertices.append(timed(lambda: live.deform(vertices={0: shapes[p]})))
        posed.append(timed(lambda: live.pose([matrix])))
        desc = description(scenes, shapes[p], faces, matrix)  # (describing the scene is not part of the route)
        t0 = time.perf_counter()
        if other is not None:
            other.close()
        closed = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        other = binding.Scene(desc)
        made = {"wall_ms": closed + 1e3 * (time.perf_counter() - t0), "destroy_ms": closed}
        created.append(made)
    assert live.n_objects == other.n_objects
    other.close()
    result["bones_deform"], result["vertices_deform"] = medians(by_bones), medians(by_vertices)
    result["pose"], result["destroy_and_create"] = medians(posed), medians(created)
    result["allocations_first_last"] = [by_bones[0]["allocations"], by_vertices[-1]["allocations"]]

    # the kernel alone: device time between two events around its launch, bytes from the derivation
    kernel = {}
    for name, n_bones, kk in (("lds", args.bones, k), ("cache", 1024, k), ("lds_k8", args.bones, 8), ("cache_k8", 1024, 8)):
        b, w = rig(verts, n_bones, kk)
        live.bind_skin(0, b, w, n_bones=n_bones)
        table = bones(n_bones, 1)
        live.deform(bones={0: table})
        ms = statistics.median(live.deform(bones={0: table})["skin_ms"] for _ in range(repeat))
        moved = len(verts) * (24 + 8 * kk) + 48 * n_bones
        kernel[name] = {"bones": n_bones, "influences": kk, "skin_ms": ms, "bytes": moved, "bytes_per_s": moved / (ms * 1e-3),
                        "fraction_of_copy_bandwidth": moved / (ms * 1e-3) / COPY_BANDWIDTH}
    live.close()
    result["skin_kernel"] = kernel
    result["ratio_create_over_bones_deform"] = result["destroy_and_create"]["wall_ms"] / result["bones_deform"]["wall_ms"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
