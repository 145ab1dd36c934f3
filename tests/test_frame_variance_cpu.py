"""CPU checks of the variance map of a frame and its measured preview (pt_frame_get_variance, pt_frame_preview_measured,
include/pt_frame_variance.h; binding.Frame.variance / preview_measured; FrameRender::variance / previewMeasured): the
refusals that need no device, the formula's restatement by hand and against the oracle's estimator, the unit of the batch means, and the
interface layers.  (The symbols and their declarations: tests/test_denoise_measured_cpu.py.)"""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build, build_host, scenes
from tests import denoise_measured_ref as mr
from tests import noise_ref, preview_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1
F = np.float32
SEED = 4711


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def test_refusals_need_no_device(lib):
    dummy = C.create_string_buffer(4096)  # (never dereferenced: every check below fails before the frame is used)
    frame = C.c_void_p(C.addressof(dummy))
    buf = np.zeros(16, F)
    ptr = C.c_void_p(buf.ctypes.data)
    assert lib.pt_frame_get_variance(None, ptr) == PT_ERR_INVALID
    assert b"null" in lib.pt_last_error()
    assert lib.pt_frame_get_variance(frame, None) == PT_ERR_INVALID
    good = binding.DenoiseMeasuredParams()
    lib.pt_denoise_measured_params_default(C.byref(good))
    assert lib.pt_frame_preview_measured(None, ptr, C.byref(good), ptr, None) == PT_ERR_INVALID
    assert lib.pt_frame_preview_measured(frame, None, C.byref(good), ptr, None) == PT_ERR_INVALID
    assert lib.pt_frame_preview_measured(frame, ptr, C.byref(good), None, None) == PT_ERR_INVALID
    for sm in (-1e-9, float("inf"), float("nan")):
        bad = binding.DenoiseMeasuredParams()
        lib.pt_denoise_measured_params_default(C.byref(bad))
        bad.sigma_measured = sm
        assert lib.pt_frame_preview_measured(frame, ptr, C.byref(bad), ptr, None) == PT_ERR_INVALID, sm
        assert b"sigma" in lib.pt_last_error()
    bad = binding.DenoiseMeasuredParams()
    lib.pt_denoise_measured_params_default(C.byref(bad))
    bad.base.iterations = 11
    assert lib.pt_frame_preview_measured(frame, ptr, C.byref(bad), ptr, None) == PT_ERR_INVALID
    assert dummy.raw == bytes(4096) and (buf == 0).all()


def test_pixel_variance_by_hand():
    # two batch means 1 and 3 per channel: M2 = 2, sample variance 2 / 1 = 2, variance of their mean 2 / 2 = 1
    count, m2 = np.array([4, 5, 3, 0, 4, 4, 4, 6]), np.full((8, 4), 2, F)
    m2[4, 1] = np.nan
    m2[5, 2] = F(-1e-9)
    m2[6, 0] = np.inf
    m2[7] = (3, 6, 12, 99)  # three batch means: v = (3 / 2) / 3, ...
    v = mr.pixel_variance(count, m2, 2)
    assert v.dtype == F and v.shape == (8, 4)
    assert v[0].tolist() == [1, 1, 1, 2] and v[1].tolist() == [1, 1, 1, 2]
    assert (v[2:7] == 0).all()  # one batch mean, none, NaN, negative, infinite: unrated
    assert v[7].tolist() == [(F(3) / F(2)) / F(3), (F(6) / F(2)) / F(3), (F(12) / F(2)) / F(3), 3]
    assert mr.rated(v).tolist() == [True, True, False, False, False, False, False, True]
    big = mr.pixel_variance([4], np.full((1, 4), 3e38, F), 2)  # (M2 / 1) / 2 stays finite; M2 itself at the top of the range does too
    assert np.isfinite(big).all() and big[0, 3] == 2


def test_restatement_against_the_oracles_estimator(oracle_lib):
    """The Cornell box at 32 x 32, min 8 / max 64 samples (batches of 2), 16 samples per pixel: the restated variance of the mean from the
    estimator's M2 against the float64 sample variance of the batch means themselves, formed here from the oracle's samples; and the unit
    -- the mean of the batch means is the preview colour pixel_value / collected_sample_count."""
    sc, cam = scenes.cornell_scene(32, 32)
    opt = scenes.options(32, 32, 8, 64)
    per_batch = noise_ref.stats_sample_count(opt)
    assert per_batch == 2
    h = oracle_lib.scene_create(sc)
    try:
        ys, xs = (a.ravel() for a in np.mgrid[0:32, 0:32])
        draws = np.full(len(xs), 16)
        count, mean, m2, accepted = noise_ref.batch_stats(h, cam, opt, SEED, xs, ys, draws, binding.pixel_seed, binding.seed_to_state)
        raw = preview_ref.raw_preview(h, cam, opt, SEED, xs, ys, draws, binding.pixel_seed, binding.seed_to_state)
        # the batch means in float64, from the samples
        half = F(0.5)
        xy = np.stack([F(2) * ((xs.astype(F) + half) / F(32) - half), -(F(2) * ((ys.astype(F) + half) / F(32) - half))], axis=1).astype(F)
        states = np.array([binding.seed_to_state(binding.pixel_seed(SEED, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
        batches = [[] for _ in xs]
        open_batch = [[] for _ in xs]
        for _ in range(16):
            rgba, col, states = h.get_sample(cam, opt, xy, states)
            for i in np.nonzero(col != 0)[0]:
                open_batch[i].append(rgba[i, :3].astype(np.float64))
                if len(open_batch[i]) == per_batch:
                    batches[i].append(np.mean(open_batch[i], axis=0))
                    open_batch[i] = []
    finally:
        h.close()
    use = ~accepted & (count == 16)  # every sample collected and the pixel still running: eight whole batches
    assert use.sum() >= 512
    v = mr.pixel_variance(count, m2, per_batch)
    assert (v[use, 3] == 8).all()
    want = np.array([np.var(np.array(b), axis=0, ddof=1) / len(b) if len(b) >= 2 else np.zeros(3) for b in batches])
    assert all(len(batches[i]) == 8 for i in np.nonzero(use)[0])
    scale = want[use].max(axis=1, keepdims=True) + 1e-12
    err = np.abs(v[use, :3] - want[use]) / scale
    print("variance of the mean: largest difference %.3g of the pixel's largest channel" % err.max())
    assert err.max() <= 1e-4  # (fp32 Welford over 8 batch means against float64 two-pass)
    # the unit: the mean of the 8 batch means is the preview colour
    centre = np.array([np.mean(np.array(batches[i]), axis=0) for i in np.nonzero(use)[0]])
    np.testing.assert_allclose(raw[use, :3], centre, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(mean[use, :3], centre, rtol=1e-5, atol=1e-7)


def test_binding_methods():
    for cls in (binding.Frame, binding.ViewsFrame):
        assert list(inspect.signature(cls.variance).parameters) == ["self"]
        assert list(inspect.signature(cls.preview_measured).parameters) == ["self", "params"]
    frame = binding.Frame.__new__(binding.Frame)
    frame._h = None
    for call in (frame.variance, frame.preview_measured):
        with pytest.raises(ValueError):
            call()
    frame._h = C.c_void_p(1)
    frame.image = np.zeros((2, 2, 4), F)
    with pytest.raises(ValueError):
        frame.preview_measured({"sigma": 1.0})  # (refused before the library sees the handle)
    frame._h = None


def test_cpp_headers_declare_the_methods(tmp_path):
    src = tmp_path / "only_headers.cpp"
    src.write_text("#include <PathTrace/frame_render.h>\n"
                   "std::vector<float> (FrameRender::*a)() const = &FrameRender::variance;\n"
                   "void (FrameRender::*b)(Image<> &, std::vector<std::int32_t> *, const pt_denoise_measured_params *) const = &FrameRender::previewMeasured;\n"
                   "int main() { return a == nullptr || b == nullptr; }\n")
    subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_cpp_library_defines_the_methods():
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    assert "FrameRender::variance() const" in out
    assert "FrameRender::previewMeasured(" in out
