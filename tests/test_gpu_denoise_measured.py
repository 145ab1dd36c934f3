"""The measured form of the denoiser (pt_denoise_measured_run) on the synthetic frames of tests/denoise_measured_cases.py,
whole runs and one kernel at a time, through the test-only probe (tests/hip/denoise_measured_probe.hip, tests/denoise_measured_probe.py).

(1) A plane that rates no pixel: the existing filter bit for bit, plain and with holes, device against device.
(2) The variance stage: the gradient bit for bit; the variance of a rated pixel bit for bit too (square roots, divisions, products and sums,
    all correctly rounded), the others within rtol 1e-4 and atol 1e-6 of the case's largest finite value, as everything below.
(3) Single a-trous launches at steps 1, 2 and 16 and whole runs against the fp32 restatement (tests/denoise_measured_ref.py); non-finite
    values equal and in the same places.
(4) Against the float64 reference (tests/denoise_measured_ref64.py): E(device) <= 4 E(restatement) per family.
(5) In place and a second run, bit for bit; the guard bands of every device buffer in every call.
(6) The preservation case: a fine texture with a tiny measured variance comes back, and is blurred away without the plane.
"""
import os

import numpy as np
import pytest

from tests import denoise_cases as dc
from tests import denoise_measured_cases as mc
from tests import denoise_measured_ref as mr
from tests import denoise_measured_ref64 as m64
from tests import denoise_ref as dr
from tests.test_gpu_denoise_units import _close
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
STEPS = (1, 2, 16)
SPATIAL = ("iterations", "sigma_luminance", "sigma_normal", "sigma_depth")


@pytest.fixture(scope="module")
def probe():
    from tests import denoise_measured_probe
    p = denoise_measured_probe.Probe(os.environ.get("PT_DENOISE_MEASURED_PROBE_LIB") or None)
    if p.device_count() < 1:
        pytest.fail("no HIP device: the denoise probe has no CPU path")
    return p


def _stages(rgba, feat, plane, samples, p):
    st = {}
    mr.denoise(rgba, feat, plane, samples, stages=st, **dict(p, iterations=0))
    return st


def test_unrated_plane_is_the_existing_filter(probe):
    for label, rgba, feat, plane, samples, p in mc.unrated():
        what = "unrated / " + label
        assert not mr.rated(plane).any(), what
        spatial = {k: p[k] for k in SPATIAL}
        want = probe.denoise(rgba, feat, spatial) if samples is None else probe.denoise_masked(rgba, feat, samples, spatial)
        assert_bits_equal(probe.denoise_measured(rgba, feat, plane, samples, p), want, what)
        assert_bits_equal(probe.denoise_measured(rgba, feat, plane, samples, p, in_place=True), want, what + ": in place")
        assert_bits_equal(probe.denoise_measured(rgba, feat, plane, samples, dict(p, sigma_measured=0.0)), want, what + ": sigma_measured 0")


@pytest.mark.parametrize("family", list(mc.FAMILIES))
def test_variance_stage(probe, family):
    worst = 0.0
    for label, rgba, feat, plane, samples, p in mc.FAMILIES[family]():
        what = "%s / %s" % (family, label)
        st = _stages(rgba, feat, plane, samples, p)
        gx, gy, var = probe.variance_measured(st["c"], st["l"], st["guide"], st["cls"], feat, plane, p["sigma_normal"], p["sigma_depth"], masked=samples is not None)
        assert_bits_equal(gx, st["gx"], what + ": gradient x")
        assert_bits_equal(gy, st["gy"], what + ": gradient y")
        use = mr.rated(plane) & ((st["cls"] & 4) == 0)
        assert_bits_equal(var[use], st["var"][use], what + ": the measured variance")
        worst = max(worst, _close(var, st["var"], what + ": variance"))
    print("%s: variance, largest difference %.3g of the case's largest value" % (family, worst))


@pytest.mark.parametrize("family", list(mc.FAMILIES))
def test_single_atrous_launches(probe, family):
    worst = dict.fromkeys(STEPS, 0.0)
    for label, rgba, feat, plane, samples, p in mc.FAMILIES[family]():
        st = _stages(rgba, feat, plane, samples, p)
        sigma = mr.pixel_sigma(plane, p["sigma_luminance"], p["sigma_measured"])
        for step in STEPS:
            what = "%s / %s: a-trous at step %d" % (family, label, step)
            args = (st["c"], st["l"], st["var"], st["guide"], st["cls"], st["gx"], st["gy"])
            wc, wl, wv = mr.atrous(*args, step, sigma, p["sigma_normal"], p["sigma_depth"])
            gc, gl, gv = probe.atrous_measured(*args, plane, step, p["sigma_luminance"], p["sigma_normal"], p["sigma_depth"], p["sigma_measured"],
                                               masked=samples is not None)
            e = max(_close(gc, wc, what + ": colour"), _close(gl, wl, what + ": luminance"), _close(gv, wv, what + ": variance"))
            worst[step] = max(worst[step], e)
    print("%s: a-trous, largest difference per step %s" % (family, {k: "%.3g" % v for k, v in worst.items()}))


@pytest.mark.parametrize("family", list(mc.FAMILIES))
def test_whole_runs(probe, family):
    worst, worst64 = 0.0, 0.0
    for label, rgba, feat, plane, samples, p in mc.FAMILIES[family]():
        what = "%s / %s" % (family, label)
        got = probe.denoise_measured(rgba, feat, plane, samples, p)
        want = mr.denoise(rgba, feat, plane, samples, **p)
        assert_bits_equal(got[..., 3], want[..., 3], what + ": alpha")
        unc = (feat[..., 0, 3] <= 0) & (True if samples is None else samples != 0)
        assert_bits_equal(got[unc], rgba[unc], what + ": uncovered pixels")
        worst = max(worst, _close(got, want, what))
        e = dc.error(got, m64.denoise(rgba, feat, plane, samples, **p), mc.ref64_mask(samples, got.shape[:2]))
        worst64 = max(worst64, e)
        assert e <= 4 * mc.E_RESTATEMENT[family], "%s: E(device) = %.3g against ref64, 4 E(restatement) = %.3g" % (what, e, 4 * mc.E_RESTATEMENT[family])
        assert_bits_equal(probe.denoise_measured(rgba, feat, plane, samples, p, in_place=True), got, what + ": in place (out == rgba)")
        assert_bits_equal(probe.denoise_measured(rgba, feat, plane, samples, p), got, what + ": a second run")
    print("%s: whole runs, largest difference %.3g of the case's largest value; E(device) against ref64 %.3g (E(restatement) %.3g)" % (
        family, worst, worst64, mc.E_RESTATEMENT[family]))


def test_preservation(probe):
    """The right half's texture has a measured variance of 1e-12: the measured form moves it by no more than the restatement says plus the
    bound of every comparison here, and the restatement says it stays (checked on the CPU).  Without the plane (B = 0) the same frame is
    blurred there: the two results differ by more than 100 times that bound, so the plane is really read."""
    rgba, feat, plane, right = mc.preservation()
    p = mc.P()
    want = mr.denoise(rgba, feat, plane, None, **p)
    got = probe.denoise_measured(rgba, feat, plane, None, p)
    _close(got, want, "preservation")
    scale = float(np.abs(want[np.isfinite(want)]).max())
    bound = 1e-4 * np.abs(want[right][:, :3]) + 1e-6 * scale
    moved = np.abs(got[right][:, :3].astype(np.float64) - rgba[right][:, :3])
    said = np.abs(want[right][:, :3].astype(np.float64) - rgba[right][:, :3])
    assert (moved <= said + bound).all()
    blurred = probe.denoise_measured(rgba, feat, np.zeros_like(plane), None, p)
    assert_bits_equal(blurred, probe.denoise(rgba, feat, {k: p[k] for k in SPATIAL}), "preservation: B = 0")
    keep = right & mc.preservation_interior()
    apart = np.abs(got[keep][:, :3].astype(np.float64) - blurred[keep][:, :3])
    print("preservation: the interior of the right half moved by %.3g at the most with the plane, by %.3g at the least without it" % (
        np.abs(got[keep][:, :3].astype(np.float64) - rgba[keep][:, :3]).max(), np.abs(blurred[keep][:, :3].astype(np.float64) - rgba[keep][:, :3]).min()))
    assert (apart > 100 * (1e-4 * np.abs(want[keep][:, :3]) + 1e-6 * scale)).all()
