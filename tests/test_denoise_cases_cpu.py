"""The synthetic denoiser cases (tests/denoise_cases.py) on the CPU: the float32 restatements against the independent float64 reference
(tests/denoise_ref64.py), the conditions the GPU tests rely on, and the dependency footprint of the filter.  No GPU."""
import os

import numpy as np
import pytest

from tests import denoise_cases as dc
from tests import denoise_ref as dr
from tests import denoise_ref64 as r64
from tests import preview_ref as pr
from tests import temporal_ref as tr

F = np.float32


@pytest.fixture(scope="module")
def plain_results():
    """{family: [(label, restatement output, ref64 output)]}, computed once."""
    out = {}
    for name, make in dc.PLAIN.items():
        out[name] = [(label, dr.denoise(rgba, feat, **p), r64.denoise(rgba, feat, **p), p) for label, rgba, feat, p in make()]
    return out


@pytest.mark.parametrize("family", list(dc.PLAIN))
def test_restatement_against_ref64(plain_results, family):
    worst = 0.0
    for label, got, want, p in plain_results[family]:
        e = dc.error(got, want, dc.ref64_mask(label, got.shape[:2], p["iterations"]))
        print("%s / %s: E(restatement) = %.3g" % (family, label, e))
        assert e <= dc.e_restatement(family, label), label
        if (family, label) not in dc.E_RESTATEMENT_CASE:
            worst = max(worst, e)
        if family != "nonfinite":
            assert np.isfinite(got).all() and np.isfinite(want).all(), label
        else:
            bad_r, bad_64 = ~np.isfinite(got).all(axis=-1), ~np.isfinite(want).all(axis=-1)
            print("    non-finite pixels: restatement %d, ref64 %d of %d" % (bad_r.sum(), bad_64.sum(), bad_r.size))
            assert bad_r.mean() <= 0.25 and bad_64.mean() <= 0.25, label
            assert (bad_r == bad_64).all(), label  # (the two follow one rule)
        assert (got[..., 3] == want[..., 3]).all(), label
    print("%s: E(restatement) = %.3g (committed %.3g)" % (family, worst, dc.E_RESTATEMENT[family]))
    assert worst <= dc.E_RESTATEMENT[family]


def test_nonfinite_family_is_what_the_issue_sets():
    for label, rgba, feat, p in dc.nonfinite():
        assert rgba.shape[:2] == (70, 70) and p["iterations"] == 2, label
        assert not (np.isfinite(rgba).all() and np.isfinite(feat).all()) or float(rgba.max()) ** 2 > np.finfo(F).max, label


def test_constant_frame_comes_back(plain_results):
    label, got, want, _ = plain_results["radiance"][0]
    assert label == "constant"
    assert np.abs(want[..., :3] - 0.75).max() <= 1e-15
    # in fp32 each pass is a normalised mean of 25 equal values: 25 products, 24 sums and a division, half an ulp each at the worst
    assert np.abs(got[..., :3] - F(0.75)).max() <= 5 * 50 * 0.5 * np.spacing(F(0.75))


def test_every_class_size_and_hole_kind_occurs():
    seen = set()
    for make in dc.PLAIN.values():
        for _, rgba, feat, _ in make():
            seen |= set(np.unique(dr.prepare(rgba, feat)[3]).tolist())
    assert seen == {0, 1, 2, 3}
    assert {(r.shape[1], r.shape[0]) for _, r, _, _ in dc.sizes()} == set(dc.SIZES)
    assert [p["iterations"] for _, r, _, p in dc.sizes() if r.shape[0] == 70] == [5]
    assert {p["iterations"] for _, _, _, p in dc.parameters()} >= {0, 1, 5, 10}
    labels = [c[0] for c in dc.masked()]
    for kind in dc.HOLE_KINDS:
        assert kind in labels, kind
    by = {c[0]: c for c in dc.masked()}
    # the kinds are what their names say
    _, rgba, feat, p, s = by["wider than footprint"]
    out = pr.denoise(rgba, feat, s, **p)
    assert (out[7, 7] == 0).all() and (out[2, 2] != 0).any()  # the middle stays empty, the rim is filled
    _, rgba, feat, p, s = by["covered, taps of another class"]
    assert (pr.denoise(rgba, feat, s, **p)[15, 16] == 0).all()
    _, rgba, feat, p, s = by["all"]
    assert (s == 0).all() and (pr.denoise(rgba, feat, s, **p) == 0).all()
    _, rgba, feat, p, s = by["class border"]
    cls = pr.prepare(rgba, feat, s)[3]
    assert len(np.unique(cls[(cls & pr.CLS_HOLE) != 0])) >= 3
    _, rgba, feat, p, s = by["none"]
    assert (s != 0).all()
    np.testing.assert_array_equal(pr.denoise(rgba, feat, s, **p).view(np.uint32), dr.denoise(rgba, feat, **p).view(np.uint32))
    for label, rgba, feat, p, s in dc.masked():
        assert np.isfinite(pr.denoise(rgba, feat, s, **p)).all(), label
    assert sorted({len(c[1]) for c in dc.views()}) == [1, 2, 5]


def test_temporal_cases_are_exact():
    """The hand-built reprojections land where the labels say, exactly in fp32, and every branch of the accumulate step is taken."""
    lengths, modes = set(), set()
    for label, rgba, feat, p, prev, cam in dc.temporal():
        c, l, guide, cls, _ = dr.prepare(rgba, feat)
        col, lum, mom, n, (mode, x0, y0, fx, fy, valid), _ = tr.accumulate(c, l, cls, feat, cam, prev, p)
        modes.add(mode)
        lengths |= set(np.unique(n).tolist())
        assert np.isfinite(col).all() and np.isfinite(mom).all(), label
        any_valid = np.any(valid, axis=0)
        covered = (cls & 1) != 0
        if label == "taps half-way":
            assert (fx[covered] == 0.5).all() and (fy[covered] == 0.5).all()
        if label == "taps px W - 0.5":
            assert (x0 == dc.TW - 1).all() and (fx == 0.5).all() and (n[:-1] == 6).all()
        if label in ("taps px -1.5", "taps px W + 0.5", "taps px -2", "taps px W + 1", "taps behind the camera"):
            assert (n == 1).all(), label
        if label == "taps px -0.5":
            assert (x0 == -1).all() and (n[1:] == 6).all()
        if label.startswith("camera, integer px"):
            assert (fx == 0).all() and (fy == 0).all() and (n[:, 0] == 1).all() and (n[:, 7] == 32).all() and (n[:, 6] == 32).all() and (n[:, 5] == 31).all()
        if label.startswith("position off by"):
            assert (n == (1 if "1.25" in label else 6)).all(), label
        if label.startswith("normal dot"):
            assert (n == (6 if ("0.75" in label or "dot 0.5" in label) else 1)).all(), label
        if label.startswith("position just") or label.startswith("normal just"):
            assert (n == (6 if "inside" in label else 1)).all(), label
        if label == "position just outside the radius":  # the fp32 operands are what the label says
            e = (feat[..., 2, :3] - prev["pos"]).astype(F)
            assert (tr._dot3(e, e) == F(1.0 + 2.0 ** -21)).all()
        if label == "position just inside the radius":
            e = (feat[..., 2, :3] - prev["pos"]).astype(F)
            assert (tr._dot3(e, e) == F(1.0 - 2.0 ** -21)).all()
        if label.startswith("kept weight"):
            want_fx = F((1048 if "under" in label else 1049) * 2.0 ** -20)
            assert (fx == want_fx).all() and (fy == 0).all()
            assert (n == (1 if "under" in label else 6)).all(), label
            assert F(1048 * 2.0 ** -20) < tr.MIN_HISTORY_WEIGHT <= F(1049 * 2.0 ** -20)
    assert modes == {tr.REPROJECT_NONE, tr.REPROJECT_IDENTICAL, tr.REPROJECT_CAMERA}
    assert lengths >= {0, 1, 2, 31, 32}


@pytest.mark.parametrize("iterations", [0, 1, 2, 3])
def test_dependency_footprint(iterations):
    """One pixel's rgb reaches exactly the pixels within Chebyshev distance R = 1 + it + 2 (2^it - 1): not farther, and as far as
    2 (2^it - 1); and no pixel that is not covered.  Between two covered classes (denoise_cases.check_footprint_two_classes): with the
    luminance term off only pixels of the changed pixel's class change; with it on the 3 x 3 prefilter of the variance, which DESIGN 4.10
    defines without a class test, lets the change cross the border, by exactly two pixels in one pass."""
    w, h = 48, 40
    cls = np.full((h, w), dc.COVERED)
    cls[:, 30:] = dc.UNCOVERED
    cls[:8, :] = dc.EMISSIVE
    rgba, feat = dc.frame(w, h, 1000, cls)
    p = dc.P(iterations=iterations)
    y, x = 20, 24
    other = rgba.copy()
    other[y, x, :3] *= F(3)
    a, b = dr.denoise(rgba, feat, **p), dr.denoise(other, feat, **p)
    changed = (a.view(np.uint32) != b.view(np.uint32)).any(axis=-1)
    ys, xs = np.mgrid[0:h, 0:w]
    dist = np.maximum(np.abs(ys - y), np.abs(xs - x))
    r = dc.footprint_radius(iterations)
    assert changed[y, x]
    assert dist[changed].max() <= r
    assert (cls[changed] == dc.COVERED).all()
    assert dist[changed].max() >= 2 * ((1 << iterations) - 1)
    for args in dc.footprint_two_classes(iterations):
        dc.check_footprint_two_classes(lambda rgba, feat, p: dr.denoise(rgba, feat, **p), *args)


def test_probe_cross_compiles(tmp_path):
    """tests/hip/denoise_probe.hip builds with the product's flags where there is no GPU."""
    from tests import denoise_probe
    lib = denoise_probe.build(force=True, lib=str(tmp_path / "libdenoise_probe.so"))
    assert os.path.getsize(lib) > 0


def test_kernel_source_on_the_host(tmp_path):
    """pt_denoise.hip itself, compiled for the host (tests/hip/host), through the device tests: every kernel and whole run of
    tests/test_gpu_denoise_units.py with the C library's expf and powf in place of the device's, guard bands included."""
    from tests import denoise_probe
    from tests import test_gpu_denoise_units as units
    probe = denoise_probe.Probe(denoise_probe.build_host(str(tmp_path / "libdenoise_probe_host.so")))
    for family in units.FAMILIES:
        units.test_prepare_gradient_variance_finish(probe, family)
        units.test_single_atrous_launches(probe, family)
    for family in dc.PLAIN:
        units.test_plain_runs(probe, family)
    units.test_masked_runs(probe)
    units.test_view_batches(probe)
    units.test_temporal(probe)
    for iterations in (0, 1, 2, 3):
        units.test_dependency_footprint(probe, iterations)
