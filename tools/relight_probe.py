"""Relighting a scene in place against the two ways there were before: destroying the scene and creating it with the
new look, and pt_scene_pose with unchanged matrices (what rebuilding everything but the upload costs; it does not change the look).
The bench mesh scene -- the box, its light quad, one point light and the stand-in mesh as ONE instance (--mesh-n 1900: 7.2 M
triangles) -- in ONE process, the three routes alternating, after a warm-up of each; every figure is the median of --repeat (5 at
least) runs with the spread (min, max) next to it.

    python tools/relight_probe.py [--mesh-n 1900] [--repeat 5]

Edits: "colour" a diffuse colour (the short cut), "light" a point light moved (the short cut), "quad" the light quad's emission scaled
(the registry rebuilt, 2 emitters), "mesh on" / "mesh off" the mesh instance switched to an emissive material and back (every triangle
of the mesh an emitter, then none).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

F = np.float32


def description(scenes, verts, faces, materials, light, mesh_material):
    """The scene under a look: materials is a list of SceneBuilder.material keyword sets (0 walls, 1 quad, 2 glass, 3 lamp)"""
    sb = scenes.SceneBuilder()
    for kw in materials:
        sb.material(**kw)
    sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), 0)
    sb.triangles(scenes.make_plane((-0.25, F(1.0) - F(0.01), -0.25), (0.25, F(1.0) - F(0.01), 0.25)), 1, cull=True)
    sb.point_light(*light)
    sb.mesh(verts, faces, np.array(scenes.DRAGON_BOX_TRANSFORM, F), mesh_material, cull=False, smooth=True)
    return sb.build()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def summary(values):
    return {"median_ms": statistics.median(values), "min_ms": min(values), "max_ms": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    from cpupathtrace_amd import binding, scenes
    repeat = max(args.repeat, 5)
    verts, faces = scenes.bumpy_sphere_vertices(args.mesh_n, args.mesh_n)
    base = [dict(diffuse=(0.8, 0.8, 0.8, 1.0)), dict(diffuse=(1, 1, 1, 1), emission=(1, 1, 1, 1)), dict(diffuse=(1, 1, 1, 1), ior=1.5, bsdf=scenes.BSDF_GLASS),
            dict(diffuse=(1, 1, 1, 1), emission=(1.0, 0.9, 0.8, 0.01))]
    light = ((-0.6, 0.7, -0.6), (0.5, 0.5, 0.4, 1.0))
    GLASS, LAMP = 2, 3

    def table(materials):
        return np.array(description(scenes, verts[:3], faces[:1], materials, light, GLASS)["materials"])

    # every edit as (relight arguments, the look it leaves: materials, light, the mesh's material); run k of an edit differs from run k - 1
    def edit(name, k):
        m = [dict(x) for x in base]
        at, mesh = light, GLASS
        if name == "colour":
            m[0] = dict(diffuse=(0.8, 0.1 + 0.1 * k, 0.3, 1.0))
        elif name == "light":
            at = ((-0.6 + 0.1 * k, 0.7, -0.6), light[1])
        elif name == "quad":
            m[1] = dict(diffuse=(1, 1, 1, 1), emission=(1, 1, 1, 1.0 + 0.5 * k))
        elif name == "mesh on":
            mesh = LAMP
        # (every call names the whole look, so that a run does not inherit the edit before it; the tables are a few hundred bytes)
        return dict(materials=table(m), point_lights=(np.array([at[0]], F), np.array([at[1]], F)), instance_materials=[(0, mesh)]), (m, at, mesh)

    live = binding.Scene(description(scenes, verts, faces, base, light, GLASS))
    identity_pose = live.pose_transforms()
    result = {"objects": live.n_objects, "faces": int(len(faces)), "repeat": repeat, "edits": {}}
    # warm-up of all three routes (the first pose grows the assembler's scratch, the first relight uploads what it keeps)
    live.pose(identity_pose)
    live.relight(**edit("quad", 0)[0])
    live.relight(**edit("mesh on", 0)[0])
    live.relight(**edit("mesh off", 0)[0])
    binding.Scene(description(scenes, verts, faces, base, light, GLASS)).close()

    other = None
    for name in ("colour", "light", "quad", "mesh on", "mesh off"):
        relit, registry, created, posed = [], [], [], []
        for k in range(1, repeat + 1):
            if name in ("mesh on", "mesh off"):  # (each run starts from the other state)
                live.relight(**edit("mesh off" if name == "mesh on" else "mesh on", k)[0])
            kwargs, look = edit(name, k)
            info, ms = timed(lambda: live.relight(**kwargs))
            relit.append(ms)
            registry.append(info.registry_ms)
            desc = description(scenes, verts, faces, *look)  # (describing the scene is not part of either route)

            def recreate():
                if other is not None:
                    other.close()
                return binding.Scene(desc)
            other, ms = timed(recreate)
            created.append(ms)
            assert other.info() == live.info() and (other.emissive()[1].view(np.uint32) == live.emissive()[1].view(np.uint32)).all(), name
            _, ms = timed(lambda: live.pose(identity_pose))
            posed.append(ms)
        result["edits"][name] = {"relight": summary(relit), "registry_ms": statistics.median(registry), "registry_rebuilt": int(info.registry_rebuilt),
                                 "n_emissive": int(info.n_emissive), "destroy_and_create": summary(created), "pose_unchanged": summary(posed)}
    if other is not None:
        other.close()
    live.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
