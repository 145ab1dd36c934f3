"""The C++ side of the light probes (Scene::lightProbes, Scene::lightProbeGrid, Scene::shadeWithLightProbes,
include/PathTrace/light_probes.h): tests/cpp/light_probes_test.cpp compiles against the PathTrace API anywhere; on the GPU the records it
prints are, bit for bit, what the Python binding returns for the same scene."""
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build_host
from tests.test_cpp_api import ROOT, SHIM, _run
from tests.test_cpp_gather import card_scene

F = np.float32
GRID = ((-0.75, -0.5, -0.25), (0.5, 0.75, 0.5), (3, 2, 2))


@pytest.fixture(scope="module")
def light_probes_test_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "light_probes_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "light_probes_test.cpp")], out, extra_includes=[SHIM], extra_flags=["-O1"])
    return out


def test_light_probes_program_compiles_and_library_exports(light_probes_test_exe):
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    for name in ("Scene::lightProbes(", "Scene::lightProbeGrid(", "Scene::shadeWithLightProbes("):
        assert out.count(name) == 1, [line for line in out.splitlines() if name in line]
    assert out.count("Scene::gather(") == 1 and out.count("Scene::getIntersection(") == 1  # (what was there stays)
    r = _run(light_probes_test_exe, skip="LightProbeScene")
    assert r.returncode == 0, r.stdout + r.stderr


def some_positions():
    k = np.arange(9)
    return np.stack([F(-1.0) + F(0.25) * k.astype(F), F(-0.5) + F(0.125) * k.astype(F), np.where(k % 3 == 0, 1.5, np.where(k % 3 == 1, 0.5, 0.0))], axis=1).astype(F)


def some_points():
    k = np.arange(11)
    pos = np.stack([F(-1.0) + F(0.25) * k.astype(F), F(-0.75) + F(0.25) * k.astype(F), F(-0.5) + F(0.125) * k.astype(F)], axis=1).astype(F)
    nrm = np.where((k % 2 == 0)[:, None], np.array([0, 0, -1], F), np.array([0, 1, 0], F)).astype(F)
    return pos, nrm


@pytest.mark.gpu
def test_the_cpp_calls_return_what_the_binding_returns(light_probes_test_exe):
    r = _run(light_probes_test_exe)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[       OK ]") == 2, r.stdout
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("RECORD "):
            _, call, index, *words = line.split()
            got.setdefault(call, {})[int(index)] = np.array([int(w, 16) for w in words], np.uint32)
    g = binding.Scene(card_scene())
    try:
        grid, nodes = g.light_probe_grid(*GRID, samples=65, epsilon=1e-3, base_seed=43)
        pos, nrm = some_points()
        want = {"points": g.light_probes(some_positions(), 65, 1e-3, 43).view(np.uint32).reshape(9, 32)[:, :30],
                "grid": nodes.ravel().view(np.uint32).reshape(12, 32)[:, :30],
                "shade": g.shade_with_light_probes(grid, nodes, pos, nrm, 0.25).view(np.uint32)}
        for call, words in want.items():
            printed = got[call]
            assert sorted(printed) == list(range(len(words))), (call, len(printed), len(words))
            for i in range(len(words)):
                assert (printed[i] == words[i]).all(), (call, i, printed[i], words[i])
    finally:
        g.close()
