"""The C++ side of the radiance calls (Scene::radiance, Scene::capture, include/PathTrace/radiance.h): tests/cpp/radiance_test.cpp
compiles against the PathTrace API anywhere; on the GPU the records it prints are, bit for bit, what the Python binding returns for the
same scene."""
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build_host
from tests.test_cpp_api import ROOT, SHIM, _run
from tests.test_cpp_gather import card_scene

F = np.float32
VIEW = ((0.1, 0.2, -1.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0))
CAPTURES = [("equirect", binding.CAPTURE_EQUIRECT, 8, 4), ("cube", binding.CAPTURE_CUBE, 18, 3), ("fisheye", binding.CAPTURE_FISHEYE, 5, 5), ("ortho", binding.CAPTURE_ORTHO, 7, 3)]


@pytest.fixture(scope="module")
def radiance_test_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "radiance_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "radiance_test.cpp")], out, extra_includes=[SHIM], extra_flags=["-O1"])
    return out


def test_radiance_program_compiles_and_library_exports(radiance_test_exe):
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    for name in ("Scene::radiance(", "Scene::capture("):
        assert out.count(name) == 1, [line for line in out.splitlines() if name in line]
    assert out.count("Scene::gather(") == 1 and out.count("Scene::lightProbes(") == 1  # (what was there stays)
    r = _run(radiance_test_exe, skip="RadianceScene")
    assert r.returncode == 0, r.stdout + r.stderr


def some_rays():
    k = np.arange(11).astype(F)
    o = np.stack([F(-0.5) + F(0.125) * k, np.full(11, 0.25, F), np.full(11, -1.0, F)], axis=1)
    d = np.stack([F(-1.25) + F(0.25) * k, F(-0.75) + F(0.125) * k, np.full(11, 1.0, F)], axis=1)
    return np.concatenate([o, d], axis=1).astype(F)


def test_the_basis_of_the_binding_is_look_at_s():
    """Capture::lookAt and binding.capture_desc state the same arithmetic: vec3::normalize multiplies by the reciprocal of the length."""
    d = binding.capture_desc(binding.CAPTURE_EQUIRECT, 8, 4, *VIEW)
    forward = (np.array(VIEW[1], F) - np.array(VIEW[0], F)).astype(F)
    length = np.sqrt(F(F(F(forward[0] * forward[0]) + F(forward[1] * forward[1])) + F(forward[2] * forward[2])))
    assert (np.array(list(d.forward), F) == forward * F(F(1.0) / length)).all()


@pytest.mark.gpu
def test_the_cpp_calls_return_what_the_binding_returns(radiance_test_exe):
    r = _run(radiance_test_exe)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[       OK ]") == 2, r.stdout
    got, counts = {}, {}
    for line in r.stdout.splitlines():
        if line.startswith("RECORD "):
            _, call, index, *words = line.split()
            got.setdefault(call, {})[int(index)] = np.array([int(w, 16) for w in words], np.uint32)
        elif line.startswith("COUNTS "):
            _, call, index, *numbers = line.split()
            counts[int(index)] = [int(v) for v in numbers]
    g = binding.Scene(card_scene())
    try:
        along = g.radiance(some_rays(), 65, 1e-3, 47)
        want = {"rays": along["value"].view(np.uint32)}
        for name, model, width, height in CAPTURES:
            desc = binding.capture_desc(model, width, height, *VIEW, fov=2.5, extent=(1.5, 0.75), jitter=True)
            want[name] = g.capture(desc, 65, 1e-3, 47)["value"].reshape(-1, 4).view(np.uint32)
        for call, words in want.items():
            printed = got[call]
            assert sorted(printed) == list(range(len(words))), (call, len(printed), len(words))
            for i in range(len(words)):
                assert (printed[i] == words[i]).all(), (call, i, printed[i], words[i])
        for i in range(len(along)):
            assert counts[i] == [int(along["samples"][i]), int(along["missed"][i]), int(along["outside"][i])], i
        assert (along["missed"] == 0).any() and (along["missed"] == 65).any()
    finally:
        g.close()
