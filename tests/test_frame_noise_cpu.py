"""CPU checks of the noise of a frame and its noise target (pt_frame_get_noise, pt_frame_set_noise_target, include/pt_frame_noise.h;
binding.Frame.set_noise_target / noise / error_map; FrameRender::setNoiseTarget / noise / errorMap / noiseTargetReached and the same on
ViewBatchRender): the symbols and their declarations, the refusals that need no device, the struct on both sides, the
histogram bin, and -- on the oracle alone -- the condition tests/test_gpu_frame_noise.py's hold test relies on."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build, build_host, scenes
from tests import noise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1
F = np.float32

DECLARATIONS = {
    "pt_frame_get_noise": "int pt_frame_get_noise(pt_frame *frame, pt_frame_noise *out, float *out_error /* [H][W] or [V][H][W], may be NULL */);",
    "pt_frame_set_noise_target": "int pt_frame_set_noise_target(pt_frame *frame, float target_error, float floor, float fraction);",
}

# the fixture of the hold test: the Cornell box at 32 x 32, min 8 / max 64 samples, and what the oracle says of it after 16 samples
SEED = 4711
HOLD_AT_OR_BELOW, HOLD_ABOVE = 312, 311


def hold_fixture():
    sc, cam = scenes.cornell_scene(32, 32)
    return sc, cam, scenes.options(32, 32, 8, 64)


def median_target(error_map):
    """T of the hold test: the median of the map's strictly positive finite errors (finished pixels are -1, unrated ones +inf)."""
    e = np.asarray(error_map, F).ravel()
    return F(np.median(e[np.isfinite(e) & (e > 0)]))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def test_symbols_are_exported_and_declared(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(binding.NOISE_EXPORTS) == set(DECLARATIONS)
    assert set(binding.NOISE_EXPORTS) <= names
    header = " ".join(open(os.path.join(ROOT, "include", "pt_frame_noise.h")).read().split())
    for name, decl in DECLARATIONS.items():
        assert " ".join(decl.split()) in header, name
    assert '#include "pt_frame_noise.h"' in open(os.path.join(ROOT, "include", "pt_hip.h")).read()


def test_refusals_need_no_device(lib):
    dummy = C.create_string_buffer(4096)  # (never dereferenced: every check below fails before the frame is used)
    frame = C.c_void_p(C.addressof(dummy))

    def set_target(f, target, floor, fraction):
        return lib.pt_frame_set_noise_target(f, C.c_float(target), C.c_float(floor), C.c_float(fraction))

    assert set_target(None, 0.1, 1e-5, 1.0) == PT_ERR_INVALID
    assert b"null frame" in lib.pt_last_error()
    for target in (-1e-9, -1.0, float("inf"), float("-inf"), float("nan")):
        assert set_target(frame, target, 1e-5, 1.0) == PT_ERR_INVALID, target
        assert b"target" in lib.pt_last_error()
    for floor in (-1e-9, float("inf"), float("nan")):
        assert set_target(frame, 0.1, floor, 1.0) == PT_ERR_INVALID, floor
        assert b"floor" in lib.pt_last_error()
    for fraction in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert set_target(frame, 0.1, 1e-5, fraction) == PT_ERR_INVALID, fraction
        assert b"fraction" in lib.pt_last_error()
    out = binding.FrameNoise()
    assert lib.pt_frame_get_noise(None, C.byref(out), None) == PT_ERR_INVALID
    assert lib.pt_frame_get_noise(frame, None, None) == PT_ERR_INVALID
    assert dummy.raw == bytes(4096)


def test_struct_layout_agrees_with_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    fields = ["target_error", "floor", "fraction", "target_reached", "streams_total", "streams_finished", "streams_rated", "streams_unrated", "streams_held",
              "max_error", "histogram"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_hip.h"\nint main(void) { printf("%zu", sizeof(pt_frame_noise));\n' +
                   "".join('printf(" %%zu", offsetof(pt_frame_noise, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    N = binding.FrameNoise
    assert [k for k, _ in N._fields_] == fields
    assert got == [C.sizeof(N)] + [getattr(N, f).offset for f in fields], got
    assert C.sizeof(binding.FrameInfo) == 80 and C.sizeof(binding.FrameProgress) == 48, "the earlier structs keep their layouts"


def test_histogram_bin():
    tiny = np.array([1e-45, 1e-39, 1.17549421e-38], F)  # the smallest and the largest denormal's neighbourhood
    assert tiny[0] > 0 and tiny[1] < np.finfo(F).tiny
    for fn in (binding.error_bin, noise_ref.error_bin):
        assert int(fn(F(0))) == 0
        assert fn(tiny[:2]).tolist() == [0, 0]
        assert int(fn(F(2.0 ** -32))) == 0 and int(fn(F(2.0 ** -31))) == 1
        assert int(fn(F(0.99999994))) == 31
        assert int(fn(F(1))) == 32 and int(fn(F(1.9999999))) == 32
        assert int(fn(F(2))) == 33
        assert int(fn(F(2.0 ** 30))) == 62 and int(fn(F(2.0 ** 31))) == 63 and int(fn(F(3e38))) == 63
        assert int(fn(F(np.inf))) == 63
    e = np.array([0, 0.5, 0.75, 1, 3, -1, np.inf], F)
    s = noise_ref.summarise(e, 0.75)
    assert (s["streams_finished"], s["streams_rated"], s["streams_unrated"], s["streams_held"], float(s["max_error"])) == (1, 5, 1, 3, 3.0)
    assert s["histogram"][[0, 31, 32, 33]].tolist() == [1, 2, 1, 1] and s["histogram"].sum() == 5
    n = binding.NoiseSummary(max_error=3.0, histogram=s["histogram"])
    assert n.percentile(20) == 2.0 ** -31 and n.percentile(60) == 1.0 and n.percentile(80) == 2.0 and n.percentile(100) == 3.0
    with pytest.raises(ValueError):
        n.percentile(0)


def test_pixel_error_restatement():
    # two batch means (1, 1, 1) and (3, 3, 3): mean 2, M2 2 per channel; stddev = sqrt(6), error = sqrt(6) / (18 + floor) / sqrt(2)
    count, mean, m2 = np.array([4, 3, 0]), np.full((3, 4), 2, F), np.full((3, 4), 2, F)
    e = noise_ref.pixel_error(count, mean, m2, 2, floor=1e-5)
    want = (np.sqrt(F(6)) / (F(18) + F(1e-5))) / np.sqrt(F(2))
    assert e.dtype == F and e[0] == want and np.isposinf(e[1]) and np.isposinf(e[2])
    assert noise_ref.pixel_error([64], np.zeros((1, 4), F), np.zeros((1, 4), F), 2, floor=0.5)[0] == 0
    assert noise_ref.stats_sample_count(scenes.options(32, 32, 8, 64)) == 2


def test_the_hold_test_has_pixels_on_both_sides(oracle_lib):
    """After 16 samples per pixel the oracle's error map of the fixture has 623 unfinished pixels, all rated; with T their median error,
    HOLD_AT_OR_BELOW = 312 lie at or below T and HOLD_ABOVE = 311 above: both groups of the hold test have at least 64 pixels."""
    sc, cam, opt = hold_fixture()
    h = oracle_lib.scene_create(sc)
    try:
        ys, xs = np.mgrid[0:32, 0:32]
        xs, ys = xs.ravel(), ys.ravel()
        count, mean, m2, accepted = noise_ref.batch_stats(h, cam, opt, SEED, xs, ys, np.full(len(xs), 16), binding.pixel_seed, binding.seed_to_state)
    finally:
        h.close()
    error = noise_ref.pixel_error(count, mean, m2, noise_ref.stats_sample_count(opt))
    error[accepted] = F(-1)
    t = median_target(error)
    unfinished = ~accepted
    below, above = int((unfinished & (error <= t)).sum()), int((unfinished & (error > t)).sum())
    print("T = %r: %d unfinished pixels at or below, %d above, %d finished" % (t, below, above, int(accepted.sum())))
    assert t > 0 and np.isfinite(error[unfinished]).all()
    assert below >= 64 and above >= 64
    assert (below, above) == (HOLD_AT_OR_BELOW, HOLD_ABOVE)


def test_binding_methods():
    for cls in (binding.Frame, binding.ViewsFrame):
        assert list(inspect.signature(cls.set_noise_target).parameters) == ["self", "target_error", "floor", "fraction"]
        assert inspect.signature(cls.set_noise_target).parameters["floor"].default == 1e-5
        assert inspect.signature(cls.set_noise_target).parameters["fraction"].default == 1.0
        assert list(inspect.signature(cls.noise).parameters) == ["self"] and list(inspect.signature(cls.error_map).parameters) == ["self"]
    frame = binding.Frame.__new__(binding.Frame)
    frame._h = None
    for call in (lambda: frame.set_noise_target(0.1), frame.noise, lambda: frame.error_map()):
        with pytest.raises(ValueError):
            call()
    frame._h = C.c_void_p(1)
    for args in ((-1.0,), (float("nan"),), (0.1, -1.0), (0.1, 1e-5, 0.0), (0.1, 1e-5, 1.5)):
        with pytest.raises(ValueError):
            frame.set_noise_target(*args)  # (refused before the library sees the handle)
    frame._h = None


def test_cpp_headers_declare_the_methods(tmp_path):
    src = tmp_path / "only_headers.cpp"
    body = ""
    for k, cls in enumerate(("FrameRender", "ViewBatchRender")):
        body += ("void (%s::*a%d)(float, float, float) = &%s::setNoiseTarget;\npt_frame_noise (%s::*b%d)() const = &%s::noise;\n"
                 "std::vector<float> (%s::*c%d)() const = &%s::errorMap;\nbool (%s::*d%d)() const = &%s::noiseTargetReached;\n" % ((cls, k, cls) * 4))
    src.write_text("#include <PathTrace/frame_render.h>\n#include <PathTrace/view_batch_render.h>\n" + body +
                   "int main() { return a0 == nullptr || b0 == nullptr || c0 == nullptr || d0 == nullptr || a1 == nullptr || b1 == nullptr || c1 == nullptr || d1 == nullptr; }\n")
    subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_cpp_program_compiles_and_links(tmp_path):
    exe = str(tmp_path / "frame_noise_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "frame_noise_test.cpp")], exe, extra_flags=["-O1"])
    assert os.path.exists(exe)
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    for cls in ("FrameRender", "ViewBatchRender"):
        for name in ("setNoiseTarget(float, float, float)", "noise() const", "errorMap() const", "noiseTargetReached() const"):
            assert cls + "::" + name in out, (cls, name)
