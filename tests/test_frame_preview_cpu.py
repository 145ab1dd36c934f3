"""CPU checks of the preview of an unfinished frame (pt_frame_preview, binding.Frame.preview, FrameRender::preview): the symbol, the argument
checks that need no device, the C++ header and test program compile, and properties of the hole-aware restatement (tests/preview_ref.py)
the GPU filter is checked against."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build, build_host
from tests import denoise_ref, preview_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    build.build()
    lib = binding.load()
    lib.pt_frame_preview.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def test_symbol_is_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(binding.PREVIEW_EXPORTS) <= names
    assert set(binding.PREVIEW_EXPORTS) <= set(binding.EXPORTS)
    header = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert "int pt_frame_preview(pt_frame *frame, const float *image, const pt_denoise_params *denoise, float *out_rgba, int32_t *out_samples);" in header


def test_preview_refuses_bad_arguments(lib):
    dummy = C.create_string_buffer(4096)  # (never dereferenced as a frame: every check below fails before the frame is read)
    img = np.zeros((4, 4, 4), np.float32)
    out = np.zeros_like(img)
    samples = np.zeros((4, 4), np.int32)
    P = binding._ptr

    def call(frame=C.addressof(dummy), image=img, params=None, o=out, s=samples):
        return lib.pt_frame_preview(frame, P(image), C.addressof(params) if params is not None else None, P(o), P(s))

    def params(**kw):
        p = binding.DenoiseParams(5, 32.0, 128.0, 1.0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad = [call(frame=None), call(image=None), call(o=None), call(frame=None, image=None, o=None),
           call(params=params(iterations=-1)), call(params=params(iterations=11)), call(params=params(sigma_luminance=-1.0)),
           call(params=params(sigma_normal=math.nan)), call(params=params(sigma_depth=math.inf))]
    assert bad == [PT_ERR_INVALID] * len(bad), bad
    assert b"iterations" in lib.pt_last_error() or b"sigma" in lib.pt_last_error()


def test_cpp_header_declares_preview(tmp_path):
    src = tmp_path / "only_header.cpp"
    src.write_text("#include <PathTrace/frame_render.h>\n"
                   "void (FrameRender::*p)(Image<> &, std::vector<std::int32_t> *, const pt_denoise_params *) const = &FrameRender::preview;\n"
                   "int main() { return p == nullptr; }\n")
    subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_cpp_program_compiles_and_links(tmp_path):
    exe = str(tmp_path / "frame_preview_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "frame_preview_test.cpp")], exe, extra_flags=["-O1"])
    assert os.path.exists(exe)
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    assert "FrameRender::preview(Image<Color<float> >&, std::vector<int, std::allocator<int> >*, pt_denoise_params const*) const" in out


# ---- properties of the restatement ---------------------------------------------------------------------------------------------------

def _scene_features(h, w):
    """Synthetic features with every class: a plane whose left third faces +x and the rest +z, t rising along x, an emissive patch and
    uncovered top rows."""
    feat = np.zeros((h, w, 3, 4), np.float32)
    feat[..., 0, :3] = (0.5, 0.25, 0.8)
    feat[..., 0, 3] = 1.0
    feat[..., 1, :3] = (0.0, 0.0, 1.0)
    feat[:, : w // 3, 1, :3] = (1.0, 0.0, 0.0)
    feat[..., 1, 3] = 2.0 + 0.01 * np.arange(w, dtype=np.float32)[None, :]
    feat[h // 2: h // 2 + 3, w // 2: w // 2 + 4, 2, 3] = 0.9  # emissive
    feat[:3] = 0.0  # no ray hit
    return feat


def _noisy(h, w, seed=11):
    rng = np.random.default_rng(seed)
    rgba = np.ones((h, w, 4), np.float32)
    rgba[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    return rgba


@pytest.mark.parametrize("params", [{}, {"iterations": 0}, {"iterations": 3, "sigma_luminance": 0.0}, {"iterations": 5, "sigma_depth": 0.0}])
def test_without_holes_the_restatement_is_denoise_bit_for_bit(params):
    h, w = 40, 56
    feat, rgba = _scene_features(h, w), _noisy(h, w)
    samples = np.full((h, w), -1, np.int32)
    samples[5:9, 7:20] = 17  # parked pixels are no holes either
    want = denoise_ref.denoise(rgba, feat, **params)
    got = preview_ref.denoise(rgba, feat, samples, **params)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_a_hole_among_valid_pixels_is_filled():
    h, w = 32, 32
    feat, rgba = _scene_features(h, w), _noisy(h, w)
    samples = np.full((h, w), -1, np.int32)
    samples[20:23, 24:27] = 0  # a 3 x 3 hole on the +z plane
    samples[10, 2] = 0         # one on the +x part
    samples[1, 5] = 0          # one where no ray hit
    rgba[samples == 0] = 0.0
    out = preview_ref.denoise(rgba, feat, samples)
    hole = samples == 0
    assert (out[hole, 3] == 1.0).all()
    assert (out[hole, :3] > 0.0).all() and np.isfinite(out[hole]).all()
    # a filled hole lies among its neighbours
    ring = out[19:24, 23:28, :3].reshape(-1, 3)
    assert (out[21, 25, :3] >= ring.min(axis=0) * 0.5).all() and (out[21, 25, :3] <= ring.max(axis=0) * 2.0).all()


def test_a_hole_block_wider_than_the_footprint_stays_empty():
    h, w = 128, 128
    feat, rgba = _scene_features(h, w), _noisy(h, w)
    samples = np.full((h, w), -1, np.int32)
    samples[20:110, 20:110] = 0  # its centre is 45 pixels from a valid one; 5 passes reach 2 * 16 = 32 at most
    rgba[samples == 0] = 0.0
    out = preview_ref.denoise(rgba, feat, samples)
    assert (out[60:70, 60:70] == 0.0).all(), "the centre of the block was filled"
    assert (out[20, 20:110, 3] == 1.0).all(), "the block's edge was not filled"


def test_holes_are_never_read():
    h, w = 48, 48
    feat, rgba = _scene_features(h, w), _noisy(h, w)
    samples = np.full((h, w), -1, np.int32)
    samples[10:14, 30:33] = 0
    samples[25, 5:9] = 0
    samples[40:, 40:] = 0
    hole = samples == 0
    a = rgba.copy()
    a[hole] = 0.0
    b = rgba.copy()
    b[hole] = np.random.default_rng(2).uniform(-5.0, 50.0, (int(hole.sum()), 4)).astype(np.float32)
    out_a = preview_ref.denoise(a, feat, samples)
    out_b = preview_ref.denoise(b, feat, samples)
    assert (out_a[~hole].view(np.uint32) == out_b[~hole].view(np.uint32)).all()
    # and the holes' own fill depends on their neighbours only
    assert (out_a[hole].view(np.uint32) == out_b[hole].view(np.uint32)).all()
    # while a change of a valid pixel does reach its neighbours
    c = a.copy()
    c[30, 30, :3] += 10.0
    assert not (preview_ref.denoise(c, feat, samples)[29, 30] == out_a[29, 30]).all()


def test_a_frame_of_holes_stays_empty():
    h, w = 16, 24
    feat = _scene_features(h, w)
    out = preview_ref.denoise(np.zeros((h, w, 4), np.float32), feat, np.zeros((h, w), np.int32))
    assert (out == 0.0).all()
