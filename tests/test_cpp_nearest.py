"""The C++ side of the nearest-surface queries (Scene::nearest, Scene::distanceGrid, include/PathTrace/nearest.h):
tests/cpp/nearest_test.cpp compiles against the PathTrace API anywhere and runs on the GPU."""
import os
import subprocess

import pytest

from cpupathtrace_amd import build_host
from tests.test_cpp_api import ROOT, SHIM, _run


@pytest.fixture(scope="module")
def nearest_test_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "nearest_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "nearest_test.cpp")], out, extra_includes=[SHIM], extra_flags=["-O1"])
    return out


def test_nearest_program_compiles_and_library_exports(nearest_test_exe):
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    assert out.count("Scene::nearest(") == 1 and out.count("Scene::distanceGrid(") == 1, [line for line in out.splitlines() if "Scene::nearest" in line or "distanceGrid" in line]
    assert out.count("Scene::pick(") == 1 and out.count("Scene::getIntersection(") == 1  # (what was there stays)
    r = _run(nearest_test_exe, skip="NearestScene")
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_nearest_program_on_gpu(nearest_test_exe):
    r = _run(nearest_test_exe)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[       OK ]") == 2, r.stdout
