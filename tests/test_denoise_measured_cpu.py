"""The measured form of the denoiser (pt_denoise_measured) on the CPU: the float32 restatement
(tests/denoise_measured_ref.py) against the existing restatements where the plane rates no pixel and against the float64 reference
(tests/denoise_measured_ref64.py) on the families of tests/denoise_measured_cases.py, the kernels' own source compiled for the host
through the device tests, the preservation case, and the entry points' symbols, defaults and refusals.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build
from tests import denoise_cases as dc
from tests import denoise_measured_cases as mc
from tests import denoise_measured_ref as mr
from tests import denoise_measured_ref64 as m64
from tests import denoise_ref as dr
from tests import preview_ref as pr
from tests.util import assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1
F = np.float32

DECLARATIONS = {
    "pt_denoise_measured_params_default": "int pt_denoise_measured_params_default(pt_denoise_measured_params *out);",
    "pt_frame_get_variance": "int pt_frame_get_variance(pt_frame *frame, float *out_var /* [H][W][4] */);",
    "pt_denoise_measured": "int pt_denoise_measured(int device, const float *rgba, const float *features, const float *variance, const int32_t *mask /* may be NULL */, "
                           "int32_t width, int32_t height, const pt_denoise_measured_params *params, float *out_rgba);",
    "pt_denoise_measured_device": "int pt_denoise_measured_device(int device, const float *d_rgba, const float *d_features, const float *d_variance, "
                                  "const int32_t *d_mask /* may be NULL */, int32_t width, int32_t height, const pt_denoise_measured_params *params, "
                                  "float *d_out_rgba, void *stream);",
    "pt_frame_preview_measured": "int pt_frame_preview_measured(pt_frame *frame, const float *image, const pt_denoise_measured_params *params, float *out_rgba, "
                                 "int32_t *out_samples);",
}


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


@pytest.fixture(scope="module")
def results():
    """{family: [(label, restatement output, ref64 output, samples)]}, computed once."""
    return {name: [(label, mr.denoise(rgba, feat, plane, s, **p), m64.denoise(rgba, feat, plane, s, **p), s) for label, rgba, feat, plane, s, p in make()]
            for name, make in mc.FAMILIES.items()}


def test_unrated_plane_is_the_existing_restatement():
    for label, rgba, feat, plane, samples, p in mc.unrated():
        spatial = {k: p[k] for k in dr.DEFAULTS}
        want = dr.denoise(rgba, feat, **spatial) if samples is None else pr.denoise(rgba, feat, samples, **spatial)
        assert_bits_equal(mr.denoise(rgba, feat, plane, samples, **p), want, label)


@pytest.mark.parametrize("family", list(mc.FAMILIES))
def test_restatement_against_ref64(results, family):
    worst = 0.0
    for label, got, want, samples in results[family]:
        e = dc.error(got, want, mc.ref64_mask(samples, got.shape[:2]))
        print("%s / %s: E(restatement) = %.3g" % (family, label, e))
        worst = max(worst, e)
        assert np.isfinite(got).all() and np.isfinite(want).all(), label
        assert (got[..., 3] == want[..., 3]).all(), label
        if samples is not None:
            assert ((got == 0).all(axis=-1) == (want == 0).all(axis=-1))[samples != 0].all(), label
    print("%s: E(restatement) = %.3g (committed %.3g)" % (family, worst, mc.E_RESTATEMENT[family]))
    assert worst <= mc.E_RESTATEMENT[family]


def test_the_families_are_what_the_issue_sets():
    assert {(c[1].shape[1], c[1].shape[0]) for c in mc.rated_all()} == set(mc.SIZES) == {(1, 1), (1, 40), (40, 1), (3, 3), (17, 33), (48, 40), (70, 70)}
    assert [c[5]["iterations"] for c in mc.rated_all() if c[1].shape[0] == 70] == [5]
    for c in mc.unrated():
        assert not mr.rated(c[3]).any(), c[0]
    assert any(c[4] is not None for c in mc.unrated()) and any(c[4] is None for c in mc.unrated())
    for c in mc.rated_all():
        assert mr.rated(c[3]).all(), c[0]
    assert [c[0] for c in mc.patterns()] == ["%s/%d" % (k, p) for k in ("checker", "columns") for p in (1, 2, 4)]
    for c in mc.patterns():
        r = mr.rated(c[3])
        assert r.any() and not r.all(), c[0]
    by = {c[0]: c for c in mc.borders()}
    _, rgba, feat, plane, s, p = by["holes, rated next to them only"]
    assert (s == 0).any() and mr.rated(plane)[s != 0].any() and not mr.rated(plane)[s != 0].all()
    assert set(np.unique(dr.prepare(rgba, feat)[3]).tolist()) == {0, 1, 2, 3}
    vals = {c[0]: c for c in mc.values()}
    for name, v in (("0", 0.0), ("denormal", float(mc.DENORMAL)), ("1e-30", float(F(1e-30))), ("1e30", float(F(1e30)))):
        assert (vals["v %s everywhere" % name][3][..., :3] == F(v)).all()
    assert 0 < mc.DENORMAL < np.finfo(F).tiny
    for a in (0.0, 0.0099, 0.01, 1.0):
        assert (vals["albedo %g" % a][2][..., 0, :3] == F(a)).any()
    assert set(np.unique(vals["B = 1 and B = 2"][3][..., 3]).tolist()) == {1.0, 2.0}
    r = mr.rated(vals["B = 1 and B = 2"][3])
    assert (r == (vals["B = 1 and B = 2"][3][..., 3] == 2)).all()
    for c in mc.nonfinite():
        for y, x in mc.NONFINITE_AT:
            assert mr.rated(c[3])[y, x] == (c[0] in ("v -0", "B inf")), c[0]  # (-0 is not negative; B = inf is at least 2)
        assert mr.rated(c[3]).sum() >= c[3].shape[0] * c[3].shape[1] - len(mc.NONFINITE_AT)
    assert {c[5]["sigma_measured"] for c in mc.parameters()} >= {0.0, 1.0, 32.0}


def test_measured_variance_by_hand():
    # one covered pixel of albedo (0.5, 0.25, 0.001): s = (sqrt(0.04) / 0.5, sqrt(0.01) / 0.25, sqrt(1e-6) / 0.01) = (0.4, 0.4, 0.1)
    rgba = np.ones((1, 1, 4), F)
    feat = np.zeros((1, 1, 3, 4), F)
    feat[0, 0, 0] = (0.5, 0.25, 0.001, 1.0)
    feat[0, 0, 1] = (0, 0, -1, 3.0)
    plane = np.array([[[0.04, 0.01, 1e-6, 2.0]]], F)
    st = {}
    mr.denoise(rgba, feat, plane, None, stages=st, **mc.P(iterations=0))
    s = (F(0.2126) * (np.sqrt(F(0.04)) / F(0.5)) + F(0.7152) * (np.sqrt(F(0.01)) / F(0.25))) + F(0.0722) * (np.sqrt(F(1e-6)) / F(0.01))
    assert st["var"][0, 0] == s * s and abs(float(st["var"][0, 0]) - (0.2126 * 0.4 + 0.7152 * 0.4 + 0.0722 * 0.1) ** 2) < 1e-7
    feat[0, 0, 2, 3] = 1.0  # emissive: not demodulated, s_c = sqrt(v_c)
    mr.denoise(rgba, feat, plane, None, stages=st, **mc.P(iterations=0))
    s = (F(0.2126) * np.sqrt(F(0.04)) + F(0.7152) * np.sqrt(F(0.01))) + F(0.0722) * np.sqrt(F(1e-6))
    assert st["var"][0, 0] == s * s
    r64 = {}
    m64.denoise(rgba, feat, plane, None, stages=r64, **mc.P(iterations=0))
    assert abs(r64["var"][0, 0] - (0.2126 * 0.2 + 0.7152 * 0.1 + 0.0722 * 1e-3) ** 2) < 1e-8


def test_preservation_restated():
    """What tests/test_gpu_denoise_measured.py::test_preservation relies on: with the plane the texture of the right half stays to a few ulp
    beyond three columns from the border; without it every pixel there moves by more than a tenth."""
    rgba, feat, plane, right = mc.preservation()
    keep = right & mc.preservation_interior()
    assert keep.sum() == 40 * 20 and mr.rated(plane).all()
    with_plane = mr.denoise(rgba, feat, plane, None, **mc.P())
    without = mr.denoise(rgba, feat, np.zeros_like(plane), None, **mc.P())
    moved = np.abs(with_plane[keep][:, :3].astype(np.float64) - rgba[keep][:, :3]).max()
    blurred = np.abs(without[keep][:, :3].astype(np.float64) - rgba[keep][:, :3]).min()
    print("preservation: moved %.3g at the most with the plane, %.3g at the least without" % (moved, blurred))
    assert moved <= 8 * np.spacing(F(0.8)) and blurred > 0.1
    left = ~right
    assert np.abs(with_plane[left][:, :3].astype(np.float64) - rgba[left][:, :3]).mean() > 0.05  # (the noisy half is filtered)


def test_probe_cross_compiles(tmp_path):
    from tests import denoise_measured_probe
    lib = denoise_measured_probe.build(force=True, lib=str(tmp_path / "libdenoise_measured_probe.so"))
    assert os.path.getsize(lib) > 0


def test_kernel_source_on_the_host(tmp_path):
    """pt_denoise.hip itself, compiled for the host (tests/hip/host), through every test of tests/test_gpu_denoise_measured.py, guard bands
    included, with the C library's expf and powf in place of the device's."""
    from tests import denoise_measured_probe
    from tests import test_gpu_denoise_measured as units
    probe = denoise_measured_probe.Probe(denoise_measured_probe.build_host(str(tmp_path / "libdenoise_measured_probe_host.so")))
    units.test_unrated_plane_is_the_existing_filter(probe)
    for family in mc.FAMILIES:
        units.test_variance_stage(probe, family)
        units.test_single_atrous_launches(probe, family)
        units.test_whole_runs(probe, family)
    units.test_preservation(probe)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_declared(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(binding.VARIANCE_EXPORTS) == set(DECLARATIONS)
    assert set(binding.VARIANCE_EXPORTS) <= names
    header = " ".join(open(os.path.join(ROOT, "include", "pt_frame_variance.h")).read().split())
    for name, decl in DECLARATIONS.items():
        assert " ".join(decl.split()) in header, name
    assert '#include "pt_frame_variance.h"' in open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert not set(binding.VARIANCE_EXPORTS) & set(binding.EXPORTS)  # (EXPORTS is what pt_hip.h itself declares)


def test_defaults_and_struct(lib, tmp_path):
    p = binding.DenoiseMeasuredParams()
    assert lib.pt_denoise_measured_params_default(C.byref(p)) == 0
    assert p.base.as_dict() == binding.denoise_params_default()
    assert p.sigma_measured == mr.DEFAULTS["sigma_measured"] and binding.denoise_measured_params_default() == {k: float(v) if k != "iterations" else v for k, v in mr.DEFAULTS.items()}
    assert lib.pt_denoise_measured_params_default(None) == PT_ERR_INVALID
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_hip.h"\nint main(void) { printf("%zu %zu %zu", sizeof(pt_denoise_measured_params), '
                   'offsetof(pt_denoise_measured_params, base), offsetof(pt_denoise_measured_params, sigma_measured)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    M = binding.DenoiseMeasuredParams
    assert got == [C.sizeof(M), M.base.offset, M.sigma_measured.offset] == [20, 0, 16]


def test_refusals_need_no_device(lib):
    buf = np.zeros(4 * 12, F)
    ptr = C.c_void_p(buf.ctypes.data)
    good = binding.DenoiseMeasuredParams()
    lib.pt_denoise_measured_params_default(C.byref(good))

    def call(rgba=ptr, feat=ptr, var=ptr, w=2, h=2, params=good, out=ptr, device_form=False):
        par = None if params is None else C.byref(params)
        if device_form:
            return lib.pt_denoise_measured_device(C.c_int(0), rgba, feat, var, None, C.c_int32(w), C.c_int32(h), par, out, None)
        return lib.pt_denoise_measured(C.c_int(0), rgba, feat, var, None, C.c_int32(w), C.c_int32(h), par, out)

    for device_form in (False, True):
        for which in ("rgba", "feat", "var", "out"):
            assert call(device_form=device_form, **{which: None}) == PT_ERR_INVALID, which
            assert b"null" in lib.pt_last_error()
        for w, h in ((0, 2), (2, 0), (-1, 2), (2, -5), (1 << 15, 1 << 15)):
            assert call(w=w, h=h, device_form=device_form) == PT_ERR_INVALID, (w, h)
        for sm in (-1e-9, -1.0, float("inf"), float("-inf"), float("nan")):
            bad = binding.DenoiseMeasuredParams()
            lib.pt_denoise_measured_params_default(C.byref(bad))
            bad.sigma_measured = sm
            assert call(params=bad, device_form=device_form) == PT_ERR_INVALID, sm
            assert b"sigma" in lib.pt_last_error()
        for field, v in (("iterations", -1), ("iterations", 11), ("sigma_luminance", -1.0), ("sigma_normal", float("nan")), ("sigma_depth", float("inf"))):
            bad = binding.DenoiseMeasuredParams()
            lib.pt_denoise_measured_params_default(C.byref(bad))
            setattr(bad.base, field, v)
            assert call(params=bad, device_form=device_form) == PT_ERR_INVALID, field
    assert (buf == 0).all()


def test_binding_functions():
    with pytest.raises(ValueError):
        binding.denoise_measured(np.zeros((4, 4, 4), F), np.zeros((4, 4, 3, 4), F), np.zeros((4, 4, 3), F))
    with pytest.raises(ValueError):
        binding.denoise_measured(np.zeros((4, 4, 4), F), np.zeros((4, 4, 3, 4), F), np.zeros((4, 4, 4), F), mask=np.zeros((4, 3), np.int32))
    with pytest.raises(ValueError):
        binding.denoise_measured(np.zeros((4, 4, 4), F), np.zeros((4, 4, 3, 4), F), np.zeros((4, 4, 4), F), params={"sigma": 1.0})
    with pytest.raises(binding.PtError):
        binding.denoise_measured(np.zeros((4, 4, 4), F), np.zeros((4, 4, 3, 4), F), np.zeros((4, 4, 4), F), params={"sigma_measured": -1.0})
