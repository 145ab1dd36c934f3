"""The C++ side of scenes from meshes and instances (io::loadMeshData, MeshInstance, Scene's third constructor): tests/cpp/mesh_scene_test.cpp
compiles against the PathTrace API anywhere and runs on the GPU."""
import os
import subprocess

import pytest

from cpupathtrace_amd import build_host
from tests.test_cpp_api import ROOT, SHIM, _run


@pytest.fixture(scope="module")
def mesh_test_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "mesh_scene_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "mesh_scene_test.cpp")], out, extra_includes=[SHIM], extra_flags=["-O1"])
    return out


def test_mesh_program_compiles_and_library_exports(mesh_test_exe):
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    for symbol in ("io::loadMeshData(", "pth_load_mesh_data", "Scene::Scene("):
        assert symbol in out, symbol
    assert "MeshInstance" in out  # the third constructor takes them
    r = _run(mesh_test_exe, skip="MeshScene")
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_mesh_program_on_gpu(mesh_test_exe):
    r = _run(mesh_test_exe)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[       OK ]") == 3, r.stdout
