"""The C++ side of blend shapes (Scene::bindMorphs, Scene::morph, include/PathTrace/detail/world.h):
tests/cpp/morph_scene_test.cpp compiles against the PathTrace API anywhere and runs on the GPU."""
import os
import subprocess

import pytest

from cpupathtrace_amd import build_host
from tests.test_cpp_api import ROOT, SHIM, _run


@pytest.fixture(scope="module")
def morph_test_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "morph_scene_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "morph_scene_test.cpp")], out, extra_includes=[SHIM], extra_flags=["-O1"])
    return out


def test_morph_program_compiles_and_library_exports(morph_test_exe):
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    assert out.count("Scene::morph(") == 2, [line for line in out.splitlines() if "Scene::morph" in line]
    assert out.count("Scene::bindMorphs(") == 1
    assert out.count("Scene::deform(") == 2 and out.count("Scene::pose(") == 2  # (what was there stays)
    r = _run(morph_test_exe, skip="MorphScene")
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_morph_program_on_gpu(morph_test_exe):
    r = _run(morph_test_exe)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[       OK ]") == 3, r.stdout
