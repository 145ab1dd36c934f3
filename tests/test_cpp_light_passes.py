"""The C++ side of the light-group passes (Scene::lightPasses, Scene::captureLightPasses, mixLightPasses,
include/PathTrace/light_passes.h): tests/cpp/light_passes_test.cpp compiles against the PathTrace API anywhere; on the GPU the passes, the
totals and the mixed values it prints are, bit for bit, what the Python binding returns for the same scene."""
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build_host
from tests.test_cpp_api import ROOT, SHIM, _run
from tests.test_cpp_gather import card_scene
from tests.test_cpp_radiance import VIEW

F = np.float32


@pytest.fixture(scope="module")
def light_passes_test_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "light_passes_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "light_passes_test.cpp")], out, extra_includes=[SHIM], extra_flags=["-O1"])
    return out


def test_light_passes_program_compiles_and_library_exports(light_passes_test_exe):
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    for name in ("Scene::lightPasses(", "Scene::captureLightPasses(", "mixLightPasses("):
        assert out.count(name) == 1, [line for line in out.splitlines() if name in line]
    assert out.count("Scene::radiance(") == 1 and out.count("Scene::capture(") == 1  # (what was there stays)
    r = _run(light_passes_test_exe, skip="LightPassScene")
    assert r.returncode == 0, r.stdout + r.stderr


def some_rays():
    """tests/cpp/light_passes_test.cpp's someRays"""
    k = np.arange(11).astype(F)
    o = np.stack([F(-0.5) + F(0.03125) * k, F(-0.5) + F(0.015625) * k, np.full(11, -1.0, F)], axis=1)
    return np.concatenate([o, np.tile(np.array([0.0, 0.0, 1.0], F), (11, 1))], axis=1).astype(F)


def some_gains(n_passes):
    p = np.arange(n_passes).astype(F)
    return np.stack([F(0.5) + F(0.25) * p, np.full(n_passes, 1.5, F), F(2.0) - F(0.125) * p], axis=1).astype(F)


@pytest.mark.gpu
def test_the_cpp_calls_return_what_the_binding_returns(light_passes_test_exe):
    r = _run(light_passes_test_exe)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[       OK ]") == 2, r.stdout
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("RECORD "):
            _, call, index, *words = line.split()
            got.setdefault(call, {})[int(index)] = np.array([int(w, 16) for w in words], np.uint32)
    g = binding.Scene(card_scene())
    try:
        groups = binding.light_groups(2, [], [1], split=True)
        desc = binding.capture_desc(binding.CAPTURE_FISHEYE, 5, 5, *VIEW, fov=2.5, jitter=True)
        want = {}
        for name, (passes, total) in (("rays", g.light_passes(some_rays(), groups, 65, 1e-3, 47)), ("capture", g.capture_light_passes(desc, groups, 65, 1e-3, 47))):
            passes, total = passes.reshape(-1, 6), total.reshape(-1)
            want[name + "_pass"] = np.ascontiguousarray(passes["value"]).reshape(-1, 3).view(np.uint32)
            want[name + "_total"] = np.ascontiguousarray(total["value"]).view(np.uint32)
            want[name + "_mix"] = binding.mix_light_passes(passes, some_gains(6), total).view(np.uint32)
            assert (passes["value"][:, :4] == 0).all()  # the objects emit nothing, and a point light is never seen along the ray itself
            assert name != "rays" or (passes["value"][0, 4] > 0).all()  # the first ray meets the sphere where the light reaches it: direct light of group 1
        for call, words in want.items():
            printed = got[call]
            assert sorted(printed) == list(range(len(words))), (call, len(printed), len(words))
            for i in range(len(words)):
                assert (printed[i] == words[i]).all(), (call, i, printed[i], words[i])
    finally:
        g.close()
