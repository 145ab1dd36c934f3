"""Re-posing a scene in place against destroying and creating it.  Both routes run in ONE process, alternating, after
a warm-up pose; every figure is the median of --repeat (5 at least) runs.

    python tools/pose_probe.py many     [--instances 256] [--mesh-n 120]   all instances posed: pt_scene_pose against destroy + pt_scene_create_meshes
    python tools/pose_probe.py big      [--instances 16] [--mesh-n 1900]   the same with 16 x 7.2 M faces
    python tools/pose_probe.py one      [--instances 256] [--mesh-n 120]   one moved instance among many (the subset form), against the same
    python tools/pose_probe.py assembly [--mesh-n 120]                      the assembly alone (pose_info.assembly_ms and the wall time around it)
                                                                            against the same chain inside a creation, at 16 and 256 instances
    python tools/pose_probe.py render   [--instances 256] [--mesh-n 120]   the first render (1024 x 1024, 4 spp) after a pose / of a fresh scene

The library's phases come from pt_pose_info and from its PT_DEBUG lines (tools/ingest_probe.py).  Every part prints one JSON line."""
import argparse
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from ingest_probe import CapturedStderr, base_builder, phases  # noqa: E402

F = np.float32


def matrices(scenes, grid, phase):
    """grid x grid placements of the stand-in mesh; `phase` moves and turns every one of them a little."""
    place = np.array(scenes.DRAGON_BOX_TRANSFORM, F)
    out = []
    for gy in range(grid):
        for gx in range(grid):
            a = F(0.3) * F(phase) + F(0.1) * F(gx + gy)
            turn = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]], F)
            m = (place @ turn).astype(F)
            m[:3, 3] = place[:3, 3] + np.array([F(2 * gx + 1) - F(grid), F(2 * gy + 1) - F(grid) + F(0.05) * F(phase), 0], F)
            out.append(m)
    return out


def description(scenes, verts, faces, grid, pose):
    sb, glass = base_builder(scenes, grid)
    for m in pose:
        sb.mesh(verts, faces, m, glass, cull=False, smooth=True)
    return sb.build()


def create(binding, desc):
    os.environ["PT_DEBUG"] = "1"
    with CapturedStderr() as err:
        t0 = time.perf_counter()
        scene = binding.Scene(desc)
        wall = 1e3 * (time.perf_counter() - t0)
    os.environ.pop("PT_DEBUG")
    return scene, dict(phases(err.text), wall_ms=wall)


def pose(scene, matrices_, instances=None):
    t0 = time.perf_counter()
    info = scene.pose(matrices_, instances)
    return dict(info, wall_ms=1e3 * (time.perf_counter() - t0))


def medians(runs):
    keys = [k for k in runs[0] if all(k in r for r in runs)]
    return {k: statistics.median(r[k] for r in runs) for k in keys}


def scratch_allocations(scene, matrices_):
    os.environ["PT_DEBUG"] = "1"
    with CapturedStderr() as err:
        scene.pose(matrices_)
    os.environ.pop("PT_DEBUG")
    m = re.search(r"scratch allocations so far (\d+)", err.text)
    return int(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["many", "big", "one", "assembly", "render"])
    ap.add_argument("--instances", type=int, default=None)
    ap.add_argument("--mesh-n", type=int, default=None)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    from cpupathtrace_amd import binding, scenes
    repeat = max(args.repeat, 5)
    n = args.mesh_n or (1900 if args.part == "big" else 120)
    count = args.instances or (16 if args.part == "big" else 256)
    grid = int(round(count ** 0.5))
    assert grid * grid == count, "--instances must be a square"
    verts, faces = scenes.bumpy_sphere_vertices(n, n)
    result = {"part": args.part, "instances": count, "faces_per_mesh": int(len(faces)), "repeat": repeat}

    if args.part in ("many", "big", "one"):
        poses = [matrices(scenes, grid, k) for k in range(2 * repeat + 3)]
        descs = {}
        moved = count // 2 + 1

        def target(k):  # the matrices pose k leaves the scene with
            if args.part != "one":
                return poses[k]
            out = list(poses[0])
            out[moved] = poses[k][moved]
            return out

        live, _ = create(binding, description(scenes, verts, faces, grid, poses[0]))
        pose(live, poses[1])  # warm-up: the scratch is grown here
        pose(live, poses[0])
        first = scratch_allocations(live, poses[0])
        posed, created = [], []
        other = None
        for k in range(1, repeat + 1):
            if args.part == "one":
                posed.append(pose(live, [poses[k][moved]], [moved]))
            else:
                posed.append(pose(live, poses[k]))
            desc = description(scenes, verts, faces, grid, target(k))  # (describing the scene is not part of either route)
            t0 = time.perf_counter()
            if other is not None:
                other.close()
            closed = 1e3 * (time.perf_counter() - t0)
            other, info = create(binding, desc)
            info["wall_ms"] += closed
            info["destroy_ms"] = closed
            created.append(info)
        result["scratch_allocations_before"], result["scratch_allocations_after"] = first, scratch_allocations(live, target(repeat))
        result["objects"] = live.n_objects
        assert live.n_objects == other.n_objects and live.info() == other.info()
        other.close()
        live.close()
        result["pose"], result["destroy_and_create"] = medians(posed), medians(created)
        result["ratio_wall"] = result["destroy_and_create"]["wall_ms"] / result["pose"]["wall_ms"]
    elif args.part == "assembly":
        result.pop("instances")
        for c in (16, 256):
            g = int(round(c ** 0.5))
            poses = [matrices(scenes, g, k) for k in range(repeat + 2)]
            live, _ = create(binding, description(scenes, verts, faces, g, poses[0]))
            pose(live, poses[1])
            posed, created = [], []
            for k in range(1, repeat + 1):
                info = pose(live, poses[k])
                posed.append({"assembly_ms": info["assembly_ms"], "syncs": float(info["assembly_syncs"]), "pose_wall_ms": info["wall_ms"]})
                other, made = create(binding, description(scenes, verts, faces, g, poses[k]))
                other.close()
                # the assembly's own wall time is what creation spends beside its other phases
                rest = sum(made.get(x, 0.0) for x in ("host_preparation_ms", "upload_ms", "device_tree_ms", "rest_ms", "mesh_upload_ms"))
                created.append({"assembly_ms": made.get("assembly_ms", float("nan")), "assembly_wall_ms": made["wall_ms"] - rest})
            live.close()
            result["%d_instances" % c] = {"pose": medians(posed), "creation": medians(created)}
    else:
        poses = [matrices(scenes, grid, k) for k in range(repeat + 2)]
        camera = scenes.camera((0, 0, -3.0 * grid), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0)
        opt = scenes.options(1024, 1024, 4, 4)
        live, _ = create(binding, description(scenes, verts, faces, grid, poses[0]))
        live.process_job(camera, opt, base_seed=1)
        pose(live, poses[1])
        after_pose, fresh = [], []
        for k in range(1, repeat + 1):
            pose(live, poses[k])
            t0 = time.perf_counter()
            a = live.process_job(camera, opt, base_seed=1)
            after_pose.append({"first_render_ms": 1e3 * (time.perf_counter() - t0)})
            other, _ = create(binding, description(scenes, verts, faces, grid, poses[k]))
            t0 = time.perf_counter()
            b = other.process_job(camera, opt, base_seed=1)
            fresh.append({"first_render_ms": 1e3 * (time.perf_counter() - t0)})
            other.close()
            assert (a.view(np.uint32) == b.view(np.uint32)).all()
        live.close()
        result["after_pose"], result["fresh_scene"] = medians(after_pose), medians(fresh)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
