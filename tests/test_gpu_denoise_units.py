"""The denoiser kernels of pt_denoise.hip on the synthetic frames of tests/denoise_cases.py, whole runs and one kernel at a time, through
the test-only probe (tests/hip/denoise_probe.hip, tests/denoise_probe.py).

(1) Bit for bit against the restatements where the kernels use only correctly rounded operations: prepare, the gradient, finish, alpha,
    uncovered pixels, accumulate's lengths, positions, normals and no-history outputs.  NaNs in the same places.
(2) Against the fp32 restatements within rtol 1e-4 and atol 1e-6 of the case's largest finite value where expf, powf or sqrtf enter:
    the variance, single a-trous launches at steps 1, 2, 16 and 512, accumulate's blend, whole runs of all four forms.  Narrowed in one
    place: the variance of the two cases of denoise_cases.CANCELLATION_ONLY is rounding noise and is held to its order, not its value.
(3) Against the independent fp64 reference: E(device) <= 4 E(restatement) per family (denoise_cases.E_RESTATEMENT).
(4) Device against device, bit for bit: in place, masked without holes, views against each view alone, temporal without history,
    two runs, the one-pixel dependency footprint.
(5) The guard bands of every device buffer: the probe raises GuardError when one was written, in every call of every test here.
"""
import os

import numpy as np
import pytest

from tests import denoise_cases as dc
from tests import denoise_ref as dr
from tests import denoise_ref64 as r64
from tests import preview_ref as pr
from tests import temporal_ref as tr
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
STEPS = (1, 2, 16, 512)


@pytest.fixture(scope="module")
def probe():
    from tests import denoise_probe
    p = denoise_probe.Probe(os.environ.get("PT_DENOISE_PROBE_LIB") or None)  # (another build of the probe: the mutation runs of DESIGN 4.10)
    if p.device_count() < 1:
        pytest.fail("no HIP device: the denoise probe has no CPU path")
    return p


def _close(got, want, what):
    """rtol 1e-4, atol 1e-6 of the largest finite |want|; non-finite values equal and in the same places.  Returns the largest difference."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    assert_bits_equal(np.where(fin, F(0), got.astype(F)), np.where(fin, F(0), want.astype(F)), what + " (non-finite values)")
    assert np.isfinite(got[fin]).all(), what
    if not fin.any():
        return 0.0
    scale = float(np.abs(want[fin]).max())
    diff = np.abs(got[fin].astype(np.float64) - want[fin])
    bound = 1e-4 * np.abs(want[fin]) + 1e-6 * scale
    assert (diff <= bound).all(), "%s: largest difference %.3g at a bound of %.3g (%d of %d values off)" % (
        what, diff.max(), bound[np.argmax(diff - bound)], int((diff > bound).sum()), diff.size)
    return float(diff.max() / scale) if scale > 0 else 0.0


def _stages(rgba, feat, p, samples=None):
    """The restatement's intermediate arrays up to the variance."""
    if samples is None:
        c, l, guide, cls, factor = dr.prepare(rgba, feat)
        gx, gy = dr.gradient(guide, cls)
        var = dr.variance(l, guide, cls, gx, gy, p["sigma_normal"], p["sigma_depth"])
    else:
        c, l, guide, cls, factor = pr.prepare(rgba, feat, samples)
        gx, gy = dr.gradient(guide, cls)
        var = pr.variance(l, guide, cls, gx, gy, p["sigma_normal"], p["sigma_depth"])
    return c, l, guide, cls, gx, gy, var


def _all_cases(family):
    if family == "masked":
        return dc.masked()
    return [c + (None,) for c in dc.PLAIN[family]()]


FAMILIES = list(dc.PLAIN) + ["masked"]


# ---- one kernel at a time -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES)
def test_prepare_gradient_variance_finish(probe, family):
    worst = 0.0
    for label, rgba, feat, p, samples in _all_cases(family):
        what = "%s / %s" % (family, label)
        c, l, guide, cls, gx, gy, var = _stages(rgba, feat, p, samples)
        got = probe.prepare(rgba, feat, samples)
        for g, w, name in zip(got, (c, l, guide, cls), ("c", "l", "guide", "cls")):
            assert_bits_equal(g, w, "%s: prepare %s" % (what, name))
        ggx, ggy, gvar = probe.variance(c, l, guide, cls, p["sigma_normal"], p["sigma_depth"], masked=samples is not None)
        assert_bits_equal(ggx, gx, what + ": gradient x")
        assert_bits_equal(ggy, gy, what + ": gradient y")
        if label in dc.CANCELLATION_ONLY:  # rounding noise only: 9 taps' worth of half ulps of l^2 on either term
            noise = 2 * 9 * 0.5 * float(np.spacing(F((l * l).max())))
            assert (gvar >= 0).all() and (gvar <= noise).all() and (var <= noise).all(), what + ": variance"
        else:
            worst = max(worst, _close(gvar, var, what + ": variance"))
        # finish, given the same colour: c itself, and on the masked form the variance as the filled flag
        if samples is None:
            want = np.empty_like(rgba)
            want[..., :3] = c * dr.prepare(rgba, feat)[4]
            want[..., 3] = rgba[..., 3]
            assert_bits_equal(probe.finish(c, l, rgba, feat), want, what + ": finish")
            assert_bits_equal(probe.finish(c, l, rgba, feat, in_place=True), want, what + ": finish in place")
        else:
            flag = np.where((np.arange(var.size).reshape(var.shape) % 2) == 0, F(1), F(0))
            hole = (cls & pr.CLS_HOLE) != 0
            want = np.empty_like(rgba)
            want[..., :3] = c * dr.prepare(rgba, feat)[4]
            want[..., 3] = np.where(hole, F(1), rgba[..., 3])
            want[hole & ~(flag > 0)] = F(0)
            assert_bits_equal(probe.finish(c, l, rgba, feat, cls=cls, var=flag), want, what + ": masked finish")
    print("%s: variance, largest difference %.3g of the case's largest value" % (family, worst))


@pytest.mark.parametrize("family", FAMILIES)
def test_single_atrous_launches(probe, family):
    worst = dict.fromkeys(STEPS, 0.0)
    for label, rgba, feat, p, samples in _all_cases(family):
        c, l, guide, cls, gx, gy, var = _stages(rgba, feat, p, samples)
        for step in STEPS:
            what = "%s / %s: a-trous at step %d" % (family, label, step)
            args = (c, l, var, guide, cls, gx, gy, step, p["sigma_luminance"], p["sigma_normal"], p["sigma_depth"])
            wc, wl, wv = (dr.atrous if samples is None else pr.atrous)(*args)
            gc, gl, gv = probe.atrous(*args, masked=samples is not None)
            unc = (cls & 1) == 0 if samples is None else np.zeros(cls.shape, bool)
            assert_bits_equal(gc[unc], c[unc], what + ": uncovered pixels")
            e = max(_close(gc, wc, what + ": colour"), _close(gl, wl, what + ": luminance"), _close(gv, wv, what + ": variance"))
            worst[step] = max(worst[step], e)
    print("%s: a-trous, largest difference per step %s" % (family, {k: "%.3g" % v for k, v in worst.items()}))


# ---- whole runs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", list(dc.PLAIN))
def test_plain_runs(probe, family):
    from tests import denoise_probe
    worst, worst64 = 0.0, 0.0
    for label, rgba, feat, p in dc.PLAIN[family]():
        what = "%s / %s" % (family, label)
        got = probe.denoise(rgba, feat, p)
        want = dr.denoise(rgba, feat, **p)
        assert_bits_equal(got[..., 3], rgba[..., 3], what + ": alpha")
        unc = feat[..., 0, 3] <= 0
        assert_bits_equal(got[unc], rgba[unc], what + ": uncovered pixels")
        worst = max(worst, _close(got, want, what))
        ref = r64.denoise(rgba, feat, **p)
        e = dc.error(got, ref, dc.ref64_mask(label, got.shape[:2], p["iterations"]))
        if (family, label) not in dc.E_RESTATEMENT_CASE:
            worst64 = max(worst64, e)
        else:
            print("%s: E(device) against ref64 %.3g (the case's own E(restatement) %.3g)" % (what, e, dc.e_restatement(family, label)))
        assert e <= 4 * dc.e_restatement(family, label), "%s: E(device) = %.3g against ref64, 4 E(restatement) = %.3g" % (what, e, 4 * dc.e_restatement(family, label))
        # device against device
        assert_bits_equal(probe.denoise(rgba, feat, p, in_place=True), got, what + ": in place")
        assert_bits_equal(probe.denoise(rgba, feat, p), got, what + ": a second run")
        ones = np.ones(rgba.shape[:2], np.int32)
        assert_bits_equal(probe.denoise_masked(rgba, feat, ones, p), got, what + ": masked without holes")
        assert_bits_equal(probe.denoise_views(rgba[None], feat[None], None, p)[0], got, what + ": a batch of one view")
        tp = tr.params(spatial=p)
        h, w = rgba.shape[:2]
        none = denoise_probe.reprojection(tr.REPROJECT_NONE)
        tout, tstate = probe.temporal(rgba, feat, tp, none, denoise_probe.prev_state(h, w))
        assert_bits_equal(tout, got, what + ": temporal without a previous push")
        assert ((tstate["len"] == 1) == ~unc).all() and ((tstate["len"] == 0) == unc).all(), what
    print("%s: whole runs, largest difference %.3g of the case's largest value; E(device) against ref64 %.3g (E(restatement) %.3g)" % (
        family, worst, worst64, dc.E_RESTATEMENT[family]))


def test_masked_runs(probe):
    worst = 0.0
    for label, rgba, feat, p, samples in dc.masked():
        what = "masked / " + label
        got = probe.denoise_masked(rgba, feat, samples, p)
        want = pr.denoise(rgba, feat, samples, **p)
        worst = max(worst, _close(got, want, what))
        assert_bits_equal(got[..., 3], want[..., 3], what + ": alpha")
        assert_bits_equal(got == 0, want == 0, what + ": the holes no pass filled")
        assert_bits_equal(probe.denoise_masked(rgba, feat, samples, p, in_place=True), got, what + ": in place")
        assert_bits_equal(probe.denoise_masked(rgba, feat, samples, p), got, what + ": a second run")
    print("masked: whole runs, largest difference %.3g of the case's largest value" % worst)


def test_view_batches(probe):
    for label, rgba, feat, p, samples in dc.views():
        v = len(rgba)
        got = probe.denoise_views(rgba, feat, samples, p)
        for i in range(v):
            alone = probe.denoise(rgba[i], feat[i], p) if samples is None else probe.denoise_masked(rgba[i], feat[i], samples[i], p)
            assert_bits_equal(got[i], alone, "%s: view %d alone" % (label, i))
            if samples is not None and (samples[i] == 0).all():
                assert (got[i] == 0).all(), "%s: the all-holes view %d" % (label, i)
            want = dr.denoise(rgba[i], feat[i], **p) if samples is None else pr.denoise(rgba[i], feat[i], samples[i], **p)
            _close(got[i], want, "%s: view %d" % (label, i))
        assert_bits_equal(probe.denoise_views(rgba, feat, samples, p, in_place=True), got, label + ": in place")
        for split in range(1, v):  # a sentinel view between two parts of the batch: the probe checks it
            assert_bits_equal(probe.denoise_views(rgba, feat, samples, p, split=split), got, "%s: split at %d" % (label, split))


# ---- temporal -----------------------------------------------------------------------------------------------------------------------

def test_temporal(probe):
    from tests import denoise_probe
    worst_blend, worst_run = 0.0, 0.0
    for label, rgba, feat, p, prev, cam in dc.temporal():
        what = "temporal / " + label
        h, w = rgba.shape[:2]
        sp = p["spatial"]
        mode, origin, rows, fp = dc.reprojection_of(cam, prev, h)
        rp = denoise_probe.reprojection(mode, origin, rows, fp)
        pv = prev if prev is not None else denoise_probe.prev_state(h, w)
        # accumulate alone
        c, l, guide, cls, factor = dr.prepare(rgba, feat)
        col, lum, mom, n, _, (X, nrm) = tr.accumulate(c, l, cls, feat, cam, prev, p)
        gcol, glum, gmom, gn, gpos, gnrm = probe.accumulate(feat, c, l, cls, rp, pv, p)
        assert_bits_equal(gn, n, what + ": history length")
        assert_bits_equal(gpos[..., :3], X, what + ": position")
        assert_bits_equal(gnrm[..., :3], nrm, what + ": normal")
        assert (gpos[..., 3] == 0).all() and (gnrm[..., 3] == 0).all(), what
        fresh = n <= 1
        assert_bits_equal(gcol[fresh], c[fresh], what + ": colour without history")
        assert_bits_equal(glum[fresh], l[fresh], what + ": luminance without history")
        assert_bits_equal(gmom[fresh], np.stack([l, l * l], axis=-1).astype(F)[fresh], what + ": moments without history")
        worst_blend = max(worst_blend, _close(gcol, col, what + ": blended colour"), _close(glum, lum, what + ": blended luminance"),
                          _close(gmom, mom, what + ": blended moments"))
        # the temporal forms of the variance and of one a-trous launch, from the restatement's integrated frame
        gx, gy = dr.gradient(guide, cls)
        temporal = (n >= p["moments_min_history"]) & (n >= 2)
        var = np.where(temporal, np.fmax(F(0.0), mom[..., 1] - mom[..., 0] * mom[..., 0]), dr.variance(lum, guide, cls, gx, gy, sp["sigma_normal"], sp["sigma_depth"])).astype(F)
        ggx, ggy, gvar = probe.variance(col, lum, guide, cls, sp["sigma_normal"], sp["sigma_depth"], temporal=(n, mom, p["moments_min_history"]))
        assert_bits_equal(ggx, gx, what + ": gradient x")
        assert_bits_equal(ggy, gy, what + ": gradient y")
        _close(gvar, var, what + ": temporal variance")
        for step in (1, 2):
            args = (col, lum, var, guide, cls, gx, gy, step)
            cs, ls, vs = dr.atrous(*args, sp["sigma_luminance"], sp["sigma_normal"], sp["sigma_depth"])
            ct, lt, vt = dr.atrous(*args, p["sigma_luminance_temporal"], sp["sigma_normal"], sp["sigma_depth"])
            gc, gl, gv = probe.atrous(*args, sp["sigma_luminance"], sp["sigma_normal"], sp["sigma_depth"],
                                      temporal=(n, mom, p["moments_min_history"], p["sigma_luminance_temporal"]))
            _close(gc, np.where(temporal[..., None], ct, cs), "%s: temporal a-trous at step %d" % (what, step))
            _close(gv, np.where(temporal, vt, vs), "%s: temporal a-trous at step %d, variance" % (what, step))
        # the whole push
        state = tr.TemporalState()
        state.prev = prev
        want, wn = tr.push(state, rgba, feat, cam, p)
        got, gstate = probe.temporal(rgba, feat, p, rp, pv)
        assert_bits_equal(gstate["len"], wn, what + ": history length of the push")
        assert_bits_equal(gstate["cls"], cls, what + ": class")
        assert_bits_equal(got[..., 3], rgba[..., 3], what + ": alpha")
        worst_run = max(worst_run, _close(got, want, what), _close(gstate["col"], state.prev["col"], what + ": colour history"),
                        _close(gstate["mom"], state.prev["mom"], what + ": moments"))
        again, _ = probe.temporal(rgba, feat, p, rp, pv, in_place=True)
        assert_bits_equal(again, got, what + ": in place")
    print("temporal: accumulate's blend, largest difference %.3g; whole pushes %.3g (of the case's largest value)" % (worst_blend, worst_run))


# ---- the dependency footprint on the device -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", [0, 1, 2, 3])
def test_dependency_footprint(probe, iterations):
    """tests/test_denoise_cases_cpu.py::test_dependency_footprint on the device: the run with one pixel changed against the run without."""
    w, h = 48, 40
    cls = np.full((h, w), dc.COVERED)
    cls[:, 30:] = dc.UNCOVERED
    cls[:8, :] = dc.EMISSIVE
    rgba, feat = dc.frame(w, h, 1000, cls)
    p = dc.P(iterations=iterations)
    ys, xs = np.mgrid[0:h, 0:w]
    r = dc.footprint_radius(iterations)
    for y, x in ((20, 24), (39, 0), (15, 16)):
        other = rgba.copy()
        other[y, x, :3] *= F(3)
        a, b = probe.denoise(rgba, feat, p), probe.denoise(other, feat, p)
        changed = (a.view(np.uint32) != b.view(np.uint32)).any(axis=-1)
        dist = np.maximum(np.abs(ys - y), np.abs(xs - x))
        assert changed[y, x]
        assert dist[changed].max() <= r, (y, x)
        assert (cls[changed] == dc.COVERED).all(), (y, x)
        assert dist[changed].max() >= 2 * ((1 << iterations) - 1), (y, x)
    for args in dc.footprint_two_classes(iterations):  # two covered classes: own class only with sigma_luminance = 0, the prefilter's leak with it
        dc.check_footprint_two_classes(probe.denoise, *args)
