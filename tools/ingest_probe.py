"""Scene ingest, flat arrays against meshes and instances: wall time to a ready scene, the library's own phases, bytes
handed over and peak host RSS.

    python tools/ingest_probe.py one    [--mesh-n 1900] [--repeat 3]     one stand-in mesh in the box: pt_scene_create from flat arrays
                                                                          against pt_scene_create_meshes, medians of --repeat
    python tools/ingest_probe.py flat16 [--mesh-n 1900] [--grid 4]       grid x grid copies, flat route   (one process each, so that
    python tools/ingest_probe.py mesh16 [--mesh-n 1900] [--grid 4]       grid x grid instances, mesh route  peak RSS is that route's)
    python tools/ingest_probe.py cpp    [--mesh-n 1900]                   the C++ API on the OBJ of tools/write_standin_obj.py:
                                                                          loadMesh -> moveObjects -> Scene against loadMeshData -> Scene(instances)

The phases are the library's PT_DEBUG lines (host preparation, upload, device tree, rest; for the mesh route also mesh upload and
assembly, the latter timed with device events).  Every run prints one JSON line."""
import argparse
import json
import os
import re
import resource
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

F = np.float32

CPP = r"""
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/scene.h>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <sys/resource.h>
static double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
int main(int argc, char **argv) {
    const bool meshes = std::strcmp(argv[1], "mesh") == 0;
    mat4<float> place{};
    place.rows[0][0] = place.rows[1][1] = place.rows[2][2] = 0.01F;
    place.rows[1][3] = -0.5F;
    place.rows[3][3] = 1.0F;
    auto glass = std::make_shared<ConstantMaterialHandler>(std::make_shared<ConstantMaterial>(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.5F), std::make_shared<GlassBDF>());
    std::vector<std::unique_ptr<Object>> objects;
    std::vector<std::unique_ptr<LightSource>> lights;
    auto walls = makeBox(vec3<float>{-1.0F, -1.0F, -1.0F}, vec3<float>{1.0F, 1.0F, 1.0F});
    moveObjects(objects, walls);
    const auto t0 = std::chrono::steady_clock::now();
    double t_load = 0, t_move = 0;
    std::unique_ptr<Scene> scene;
    if(meshes) {
        auto data = std::make_shared<const io::MeshData>(io::loadMeshData(std::filesystem::path(argv[2])));
        t_load = since(t0);
        std::vector<MeshInstance> instances;
        instances.push_back(MeshInstance{data, place, false, true, glass});
        scene = std::make_unique<Scene>(std::move(objects), std::move(lights), std::move(instances));
    }
    else {
        auto mesh = io::loadMesh(std::filesystem::path(argv[2]), place, false, true);
        t_load = since(t0);
        for(auto &t : mesh) {
            t.setMaterialHandler(glass);
        }
        moveObjects(objects, mesh);
        t_move = since(t0) - t_load;
        scene = std::make_unique<Scene>(std::move(objects), std::move(lights));
    }
    const double t_ready = since(t0);
    struct rusage usage {};
    getrusage(RUSAGE_SELF, &usage);
    std::printf("{\"route\": \"%s\", \"load_s\": %.3f, \"move_objects_s\": %.3f, \"scene_s\": %.3f, \"ready_s\": %.3f, \"peak_rss_mb\": %.1f}\n", argv[1], t_load, t_move,
                t_ready - t_load - t_move, t_ready, usage.ru_maxrss / 1024.0);
    return 0;
}
"""


def peak_rss_mb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


class CapturedStderr:
    """The library's PT_DEBUG lines of the calls made inside the block (they are written to file descriptor 2 by C code)."""

    def __enter__(self):
        self.file = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.file.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.file.seek(0)
        self.text = self.file.read().decode(errors="replace")
        self.file.close()


def phases(text):
    out = {}
    m = re.search(r"host preparation ([0-9.]+) ms, upload ([0-9.]+) ms, device tree ([0-9.]+) ms, rest ([0-9.]+) ms", text)
    if m:
        out.update(zip(("host_preparation_ms", "upload_ms", "device_tree_ms", "rest_ms"), map(float, m.groups())))
    m = re.search(r"mesh upload ([0-9.]+) ms \((\d+) bytes\), assembly ([0-9.]+) ms", text)
    if m:
        out.update(mesh_upload_ms=float(m.group(1)), mesh_upload_bytes=int(m.group(2)), assembly_ms=float(m.group(3)))
    return out


def timed_scene(binding, desc):
    os.environ["PT_DEBUG"] = "1"
    with CapturedStderr() as err:
        t0 = time.perf_counter()
        scene = binding.Scene(desc)
        wall = time.perf_counter() - t0
    info = dict(phases(err.text), wall_ms=1e3 * wall, objects=scene.n_objects)
    scene.close()
    return info


def median_of(runs):
    return {k: (statistics.median(r[k] for r in runs) if isinstance(runs[0][k], float) else runs[0][k]) for k in runs[0]}


def flat_bytes(desc):
    return int(sum(desc[k].nbytes for k in ("obj_kind", "tri_pos", "tri_nrm", "tri_cull", "tri_material")))


def base_builder(scenes, grid=1):
    sb = scenes.SceneBuilder()
    half = F(grid)
    if grid == 1:
        sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)))
        light = sb.material((1, 1, 1, 1), 1.0, (1, 1, 1, 1))
        sb.triangles(scenes.make_plane((-0.25, F(1.0) - F(0.01), -0.25), (0.25, F(1.0) - F(0.01), 0.25)), light, cull=True)
    else:
        sb.triangles(scenes.make_box((-half, -half, -1.0), (half, half, 1.0)))
        light = sb.material((1, 1, 1, 1), 1.0, (1, 1, 1, 1))
        sb.triangles(scenes.make_plane((-0.25 * grid, half - F(0.01), -0.25), (0.25 * grid, half - F(0.01), 0.25)), light, cull=True)
    return sb, sb.material((1, 1, 1, 1), 1.5, bsdf=scenes.BSDF_GLASS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["one", "flat16", "mesh16", "cpp"])
    ap.add_argument("--mesh-n", type=int, default=1900)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    from cpupathtrace_amd import binding, build_host, scenes
    n = args.mesh_n
    place = np.array(scenes.DRAGON_BOX_TRANSFORM, F)
    result = {"part": args.part, "mesh_n": n}
    if args.part == "one":
        verts, faces = scenes.bumpy_sphere_vertices(n, n)
        t0 = time.perf_counter()
        pos, nrm = scenes.bumpy_sphere_mesh(n, n, place)
        result["host_expansion_s"] = time.perf_counter() - t0
        sb, glass = base_builder(scenes)
        sb.triangles(pos, glass, cull=False, normals=nrm)
        flat = sb.build()
        sb, glass = base_builder(scenes)
        sb.mesh(verts, faces, place, glass, cull=False, smooth=True)
        meshed = sb.build()
        timed_scene(binding, flat)  # warm-up: the first scene of a process pays for the runtime's start
        result["flat"] = dict(median_of([timed_scene(binding, flat) for _ in range(args.repeat)]), bytes_handed_over=flat_bytes(flat))
        result["meshes"] = dict(median_of([timed_scene(binding, meshed) for _ in range(args.repeat)]),
                                bytes_handed_over=flat_bytes(meshed) + verts.nbytes + faces.astype(np.int32).nbytes)
    elif args.part in ("flat16", "mesh16"):
        g = args.grid
        verts, faces = scenes.bumpy_sphere_vertices(n, n)
        sb, glass = base_builder(scenes, g)
        t0 = time.perf_counter()
        if args.part == "flat16":
            pos, nrm = scenes.bumpy_sphere_mesh(n, n, place)
            desc, _ = scenes.dragon_grid_scene(pos, nrm, grid=g)
            handed = flat_bytes(desc)
        else:
            for gy in range(g):
                for gx in range(g):
                    m = place.copy()  # (the flat route shifts the transformed mesh; here the shift is part of the matrix)
                    m[:3, 3] += np.array([F(2 * gx + 1) - F(g), F(2 * gy + 1) - F(g), 0], F)
                    sb.mesh(verts, faces, m, glass, cull=False, smooth=True)
            desc = sb.build()
            handed = flat_bytes(desc) + verts.nbytes + faces.astype(np.int32).nbytes
        result["describe_s"] = time.perf_counter() - t0
        result.update(timed_scene(binding, desc), bytes_handed_over=handed, instances=g * g, peak_rss_mb=peak_rss_mb())
    else:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import write_standin_obj
        with tempfile.TemporaryDirectory() as tmp:
            obj = os.path.join(tmp, "standin.obj")
            result["triangles"] = write_standin_obj.write(obj, n)
            src, exe = os.path.join(tmp, "ingest.cpp"), os.path.join(tmp, "ingest")
            open(src, "w").write(CPP)
            build_host.compile_program([src], exe, extra_flags=["-O2"])
            env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join([build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]))
            for route in ("flat", "mesh"):
                runs = [json.loads(subprocess.run([exe, route, obj], env=env, check=True, capture_output=True, text=True).stdout) for _ in range(args.repeat)]
                result[route] = median_of(runs)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
