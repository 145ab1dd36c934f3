"""Deterministic synthetic frames for the denoiser (pt_denoise.hip): what a rendered frame never shows the filter.  Each family is a
function that returns a list of cases from fixed seeds; tests/test_denoise_cases_cpu.py checks the restatements on them against the
independent float64 reference (tests/denoise_ref64.py), tests/test_gpu_denoise_units.py runs them on the device through
tests/denoise_probe.py.

  plain families  (label, rgba (H, W, 4), features (H, W, 3, 4), params)            PLAIN[name]()
  masked()        (label, rgba, features, params, samples (H, W) int32)             0 = hole
  views()         (label, rgba (V, H, W, 4), features, params, samples or None)
  temporal()      (label, rgba, features, params, prev, cam)                        prev: temporal_ref's state dict (with "cam") or None

Sizes are width x height.  Features as pt_render_features writes them: F0 = (albedo * cov, cov), F1 = (normal * cov, t * cov),
F2 = (position * cov, luminance of the emission).
"""
import numpy as np

from tests import denoise_ref as dr
from tests import temporal_ref as tr

F = np.float32
SIZES = [(1, 1), (1, 40), (40, 1), (3, 3), (15, 17), (16, 16), (17, 33), (33, 31), (48, 40), (70, 70)]
UNCOVERED, COVERED, EMISSIVE, COVERED_EMISSIVE = 0, 1, 2, 3


def P(**kw):
    return dict(dr.DEFAULTS, **kw)


def frame(w, h, seed, cls=None, coverage=1.0, albedo=None, sigma=0.5):
    """A noisy frame over a tilted plane seen head-on: log-normal radiance around the albedo, t a planar ramp, normals (0, 0, -1)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    cls = np.full((h, w), COVERED) if cls is None else np.asarray(cls)
    cov = np.where((cls & 1) != 0, np.broadcast_to(np.asarray(coverage, F), (h, w)), F(0)).astype(F)
    alb = rng.uniform(0.2, 0.9, (h, w, 3)).astype(F) if albedo is None else np.broadcast_to(np.asarray(albedo, F), (h, w, 3)).astype(F)
    t = (F(5) + F(0.125) * xs.astype(F) + F(0.0625) * ys.astype(F)).astype(F)
    feat = np.zeros((h, w, 3, 4), F)
    feat[..., 0, :3] = alb * cov[..., None]
    feat[..., 0, 3] = cov
    feat[..., 1, 2] = -cov
    feat[..., 1, 3] = t * cov
    feat[..., 2, 0] = xs * cov
    feat[..., 2, 1] = ys * cov
    feat[..., 2, 2] = t * cov
    feat[..., 2, 3] = np.where((cls & 2) != 0, F(1.5), F(0))
    rgba = np.ones((h, w, 4), F)
    rgba[..., :3] = (np.maximum(alb, F(0.05)) * np.exp(rng.normal(0, sigma, (h, w, 3)))).astype(F)
    rgba[..., 3] = np.where(cls != 0, F(1), F(0.25))
    return rgba, feat


# ---- plain families ---------------------------------------------------------------------------------------------------------------

def sizes():
    return [("%dx%d" % (w, h), *frame(w, h, 100 + i), P()) for i, (w, h) in enumerate(SIZES)]


def _pattern(w, h, kind, period):
    ys, xs = np.mgrid[0:h, 0:w]
    if kind == "checker":
        return ((xs // period + 2 * (ys // period)) % 4 + (xs // period) // 2) % 4  # all four classes, every period-th pixel another one
    if kind == "columns":
        return (xs // period) % 4
    return (ys // period) % 4


def classes():
    out = []
    for kind in ("checker", "columns", "rows"):
        for period in (1, 2, 4, 16):
            out.append(("%s/%d" % (kind, period), *frame(48, 40, 200 + period, _pattern(48, 40, kind, period)), P()))
    one = np.zeros((17, 15), int)
    one[8, 7] = COVERED
    out.append(("one covered", *frame(15, 17, 210, one), P(iterations=3)))
    out.append(("one uncovered", *frame(15, 17, 211, 1 - one), P(iterations=3)))
    edge = np.full((31, 33), COVERED)
    edge[-1, :] = COVERED_EMISSIVE
    edge[:, -1] = UNCOVERED
    edge[-1, -1] = EMISSIVE
    out.append(("last row and column", *frame(33, 31, 212, edge), P()))
    return out


def guides():
    out = []
    w, h = 33, 31
    ys, xs = np.mgrid[0:h, 0:w]

    def with_t(t, seed):
        rgba, feat = frame(w, h, seed)
        feat[..., 1, 3] = t
        feat[..., 2, 2] = t
        return rgba, feat

    out.append(("planar ramp", *frame(w, h, 300), P()))  # the gradient predicts t exactly: only the kDepthRel floor acts
    for d in (1, 2, 4, 16):
        out.append(("depth step at %d" % d, *with_t(np.where(xs >= 16, F(9), F(5)).astype(F) + np.where(ys >= 16 - d, F(2), F(0)).astype(F), 301 + d), P()))
    out.append(("t = 0", *with_t(np.zeros((h, w), F), 310), P()))
    out.append(("t = 0 in places", *with_t(np.where((xs + ys) % 3 == 0, F(0), F(4)).astype(F), 311), P()))
    normals = {"parallel": (0, 0, -1), "orthogonal": (1, 0, 0), "antiparallel": (0, 0, 1), "short": (0, 0, -0.5), "zero": (0, 0, 0),
               "nan": (np.nan, 0, -1)}
    for i, (name, nv) in enumerate(normals.items()):
        rgba, feat = frame(w, h, 320 + i)
        sel = (xs % 5 == 2) & (ys % 4 == 1)
        feat[sel, 1, :3] = np.asarray(nv, F)
        out.append(("normal " + name, rgba, feat, P()))
        if name in ("zero", "nan", "short"):
            out.append(("normal %s, sigma_normal 0" % name, rgba, feat, P(sigma_normal=0.0)))
    for cov in (0.25, 0.5, 0.75):
        cmap = np.where((xs + 2 * ys) % 7 < 3, F(cov), F(1)).astype(F)
        out.append(("coverage %g" % cov, *frame(w, h, 330, coverage=cmap), P()))
    for i, a in enumerate((0.0, 0.0099, 0.01, 1.0)):
        amap = np.where(((xs // 2 + ys) % 2 == 0)[..., None], F(a), F(0.5)).astype(F) * np.ones(3, F)
        out.append(("albedo %g" % a, *frame(w, h, 340 + i, albedo=amap), P()))
    return out


def radiance():
    out = []
    w, h = 33, 31
    rng = np.random.default_rng(400)
    rgba, feat = frame(w, h, 401, albedo=1.0)
    rgba[..., :3] = F(0.75)
    out.append(("constant", rgba.copy(), feat, P()))
    rgba = rgba.copy()
    rgba[..., :3] = np.nextafter(F(1), rng.choice([F(0), F(2)], (h, w, 3)).astype(F)).astype(F)
    out.append(("1 +- 1 ulp", rgba, feat, P()))
    rgba = rgba.copy()
    rgba[..., :3] = np.exp(rng.normal(0.0, 2 * np.log(10.0), (h, w, 3))).astype(F)  # sigma of two decades: +-3 sigma span twelve
    out.append(("log-normal, 12 decades", rgba, feat, P()))
    rgba, feat = frame(w, h, 402)
    rgba[13, 17, :3] = F(1e6)
    out.append(("firefly 1e6", rgba, feat, P()))
    rgba, feat = frame(w, h, 403)
    rgba[..., :3] -= F(0.6)
    out.append(("negative", rgba, feat, P()))
    return out


def parameters():
    out = []
    cls = _pattern(33, 31, "checker", 4)
    cls = np.where(cls == UNCOVERED, COVERED, cls)
    for it in (0, 1, 5, 10):
        out.append(("iterations %d" % it, *frame(33, 31, 500 + it, cls), P(iterations=it)))
    for name in ("sigma_luminance", "sigma_normal", "sigma_depth"):
        out.append((name + " 0", *frame(33, 31, 520, cls), P(iterations=3, **{name: 0.0})))
    out.append(("all sigmas 0", *frame(33, 31, 521, cls), P(iterations=3, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0)))
    for sn in (1.0, 128.0):
        rgba, feat = frame(33, 31, 530, cls)
        ys, xs = np.mgrid[0:31, 0:33]
        a = (xs * 0.05).astype(F)  # normals that turn across the frame
        feat[..., 1, 0], feat[..., 1, 2] = np.sin(a) * feat[..., 0, 3], -np.cos(a) * feat[..., 0, 3]
        out.append(("sigma_normal %g" % sn, rgba, feat, P(iterations=3, sigma_normal=sn)))
    return out


NONFINITE_SIZE, NONFINITE_ITERATIONS = (70, 70), 2
NONFINITE_AT = [(20, 20), (20, 39), (20, 41), (49, 10), (60, 60)]


def nonfinite():
    out = []
    w, h = NONFINITE_SIZE
    cls = np.full((h, w), COVERED)
    cls[:, 40:] = COVERED_EMISSIVE
    cls[50:, :] = UNCOVERED
    p = P(iterations=NONFINITE_ITERATIONS)
    at = NONFINITE_AT  # inside a class, either side of a class border, above and inside the uncovered
    for what, v in (("nan", np.nan), ("inf", np.inf), ("1e25", 1e25), ("-inf", -np.inf)):
        rgba, feat = frame(w, h, 600, cls)
        for y, x in at:
            rgba[y, x, 1] = F(v)
        out.append(("radiance " + what, rgba, feat, p))
    rgba, feat = frame(w, h, 601, cls)
    for y, x in at:
        feat[y, x, 1, 0] = np.nan
    out.append(("normal nan", rgba, feat, p))
    rgba, feat = frame(w, h, 602, cls)
    for y, x in at:
        feat[y, x, 0, 1] = np.nan  # albedo: the floor takes it
    out.append(("albedo nan", rgba, feat, p))
    return out


# Cases whose 3 x 3 variance is cancellation only (m2 / sw - mean^2 of all but equal values): rounding noise of the order of eps l^2, which moves
# entirely when expf is rounded differently (shown on the CPU: the restatement with exp, pow and sqrt rounded correctly from fp64 moves it
# by 1.2e-7 and 3.6e-7).  Their variance is held to that order instead of to the restatement's value; everything after it is compared as
# everywhere.
CANCELLATION_ONLY = ("constant", "1 +- 1 ulp")

PLAIN = {"sizes": sizes, "classes": classes, "guides": guides, "radiance": radiance, "parameters": parameters, "nonfinite": nonfinite}

# E(restatement) = max |x - ref64| / (|ref64| + 1e-3 mean |ref64|) over rgb, the largest of each family's cases: tests/denoise_ref.py
# against tests/denoise_ref64.py on the CPU (tests/test_denoise_cases_cpu.py prints them), rounded up to two digits.  The device is held
# to 4 x these (tests/test_gpu_denoise_units.py).  The non-finite family: over the pixels both references give finite.
E_RESTATEMENT = {"sizes": 4.7e-7, "classes": 6.5e-7, "guides": 4.1e-7, "radiance": 2.1e-5, "parameters": 2.1e-6, "nonfinite": 5.2e-7}


# The checkerboard of period 1 has pixels without a neighbour of their class in the 3 x 3 window: their variance is l * l - l * l, rounding
# noise (0 or about 1e-16 in fp64, 0 or about 1e-8 in fp32), and the luminance weight sigma_l sqrt(g) + 1e-10 of the passes is decided by that
# noise, differently in each precision (with sigma_luminance = 0 the case measures 4.5e-7).  It has a constant of its own, so that the family's
# does not hide behind it.
E_RESTATEMENT_CASE = {("classes", "checker/1"): 8.4e-4}


def e_restatement(family, label):
    return E_RESTATEMENT_CASE.get((family, label), E_RESTATEMENT[family])


def error(x, ref, mask=None):
    """E(x) of the issue, over the pixels where ref is finite (and `mask` holds)."""
    ref = np.asarray(ref, np.float64)[..., :3]
    x = np.asarray(x, np.float64)[..., :3]
    ok = np.isfinite(ref)
    if mask is not None:
        ok = ok & mask[..., None]
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        e = np.abs(x - ref) / (np.abs(ref) + 1e-3 * np.abs(ref[ok]).mean())
    return float(np.nan_to_num(e[ok], nan=np.inf).max())


def ref64_mask(label, shape, iterations):
    """Where ref64 can stand for the fp32 definition.  Everywhere, but for the 1e25 pixels: their luminance squared overflows fp32 and not
    fp64, so within their reach the two are different filters (there the fp32 restatement alone is the reference)."""
    ok = np.ones(shape, bool)
    if "1e25" in label:
        r = footprint_radius(iterations)
        for y, x in NONFINITE_AT:
            ok[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = False
    return ok


def footprint_radius(iterations):
    """How far one pixel's rgb reaches: the 3 x 3 variance, one prefilter ring per pass, two taps of 2^i per pass."""
    return 1 + iterations + 2 * ((1 << iterations) - 1)


def footprint_two_classes(iterations):
    """Frames of two covered classes either side of column 30 and the pixels to change: (cls, rgba, features, (y, x), iterations)."""
    w, h = 48, 40
    cls = np.full((h, w), COVERED)
    cls[:, 30:] = COVERED_EMISSIVE
    cls[:8, :] = EMISSIVE
    rgba, feat = frame(w, h, 1000, cls)
    return [(cls, rgba, feat, at, iterations) for at in ((20, 24), (20, 28))]


def check_footprint_two_classes(denoise, cls, rgba, feat, at, iterations):
    """`denoise(rgba, features, params)` on the frame with and without pixel `at` changed.  sigma_luminance = 0: only pixels of that pixel's
    class change, within R.  Default sigmas: the variance of `at` and of its neighbours of its class changes, and the 3 x 3 prefilter of the
    variance has no class test, so a pixel of the other covered class changes where its 3 x 3 window holds one of those: in a single pass
    within Chebyshev distance 2 of `at` and no farther (from (20, 28), two columns off the border, exactly 2), in no pass at all none; later
    passes spread it inside the other class as inside the own, so only R bounds it then."""
    y, x = at
    other = rgba.copy()
    other[y, x, :3] *= F(3)
    ys, xs = np.mgrid[0:cls.shape[0], 0:cls.shape[1]]
    dist = np.maximum(np.abs(ys - y), np.abs(xs - x))
    r = footprint_radius(iterations)

    def changed(p):
        a, b = denoise(rgba, feat, p), denoise(other, feat, p)
        return (np.asarray(a, F).view(np.uint32) != np.asarray(b, F).view(np.uint32)).any(axis=-1)

    off = changed(P(iterations=iterations, sigma_luminance=0.0))
    assert off[y, x] and (cls[off] == COVERED).all() and dist[off].max() <= r, at
    assert dist[off].max() >= 2 * ((1 << iterations) - 1), at
    on = changed(P(iterations=iterations))
    assert on[y, x] and ((cls[on] & 1) != 0).all() and dist[on].max() <= r, at
    across = on & (cls != COVERED)
    if iterations == 0:
        assert not across.any(), at
    if iterations == 1:
        assert across.any() == (x == 28) and (not across.any() or dist[across].max() == 2), at


# ---- holes ----------------------------------------------------------------------------------------------------------------------

HOLE_KINDS = ("isolated", "3x3", "wider than footprint", "class border", "corners", "all", "none", "covered, taps of another class")


def masked():
    out = []
    w, h = 33, 31
    rng = np.random.default_rng(700)
    cls = np.full((h, w), COVERED)
    cls[:, 20:] = COVERED_EMISSIVE
    cls[24:, :] = UNCOVERED

    def case(label, holes, p, cls=cls, seed=701):
        rgba, feat = frame(w, h, seed, cls)
        s = rng.integers(1, 9, (h, w)).astype(np.int32)
        s[holes] = 0
        rgba[holes] = F(7)  # (a hole's colour is 0 whatever the input holds)
        out.append((label, rgba, feat, p, s))

    z = lambda: np.zeros((h, w), bool)
    m = z(); m[10, 10] = True; m[28, 5] = True
    case("isolated", m, P())
    m = z(); m[5:8, 5:8] = True; m[26:29, 26:29] = True
    case("3x3", m, P(iterations=1))
    m = z(); m[2:13, 2:13] = True
    case("wider than footprint", m, P(iterations=1))  # one pass reaches 2 pixels: the block's middle stays empty
    case("wider than footprint, 2 passes", m, P(iterations=2))
    m = z(); m[8:12, 18:22] = True; m[22:26, 4:8] = True
    case("class border", m, P())
    m = z(); m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True; m[0:2, 0:2] = True
    case("corners", m, P(iterations=2))
    case("all", ~z(), P(iterations=2))
    case("none", z(), P())
    lone = np.zeros((h, w), int)
    lone[15, 16] = COVERED
    m = z(); m[15, 16] = True
    case("covered, taps of another class", m, P(), cls=lone)
    m = rng.random((h, w)) < 0.4
    case("random 40 %", m, P())
    for wh, hh in ((1, 1), (3, 3), (17, 15)):
        rgba, feat = frame(wh, hh, 710)
        s = np.ones((hh, wh), np.int32)
        s[hh // 2, wh // 2] = 0
        out.append(("%dx%d, centre hole" % (wh, hh), rgba, feat, P(), s))
    return out


def views():
    out = []
    w, h = 17, 33
    rng = np.random.default_rng(800)
    for v in (1, 2, 5):
        frames = [frame(w, h, 810 + i, _pattern(w, h, "checker", 4) | 1) for i in range(v)]
        rgba, feat = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
        out.append(("%d views" % v, rgba, feat, P(), None))
        s = rng.integers(0, 3, (v, h, w)).astype(np.int32)
        out.append(("%d views, holes" % v, rgba, feat, P(), s))
        if v > 1:
            s = np.ones((v, h, w), np.int32)
            s[1] = 0  # all holes, its rows within reach of its neighbours' in the stacked arrays
            out.append(("%d views, view 1 all holes" % v, rgba, feat, P(), s))
    return out


# ---- temporal -------------------------------------------------------------------------------------------------------------------

TW, TH = 16, 16  # powers of two: the reprojected coordinates below are exact in fp32


def _cam(origin):
    return {"origin": origin, "look_at": (origin[0], origin[1], origin[2] + 1.0), "up": (0.0, 1.0, 0.0), "focal_length": 1.0, "height": 2.0, "aspect_ratio": 1.0}


CAM_NOW, CAM_BEFORE = _cam((0.0, 0.0, -1.0)), _cam((0.0, 0.0, 0.0))  # CAM_BEFORE: rows (0, 0, 1), (0, 1, 0), (-1, 0, 0): px = 8 - 8 X - 1/2, py = 8 - 8 Y - 1/2 at Z = 1


def reprojection_of(cam, prev, height):
    """(mode, origin, rows, footprint) as pt_image.cpp derives them, through temporal_ref's own terms."""
    fp = float(tr.footprint(cam, height))
    if prev is None:
        return tr.REPROJECT_NONE, (0, 0, 0), np.eye(3, dtype=F), fp
    if tr._same_camera(cam, prev["cam"]):
        return tr.REPROJECT_IDENTICAL, prev["cam"]["origin"], tr.camera_rows(prev["cam"]), fp
    return tr.REPROJECT_CAMERA, prev["cam"]["origin"], tr.camera_rows(prev["cam"]), fp


def positions_for(px, py, front=True):
    """World positions that CAM_BEFORE sees at the continuous pixel (px, py) of a TW x TH image."""
    x = -((np.asarray(px, np.float64) + 0.5) / (TW / 2) - 1.0)
    y = -((np.asarray(py, np.float64) + 0.5) / (TH / 2) - 1.0)
    z = np.where(front, 1.0, -1.0) * np.ones_like(x)
    return np.stack([x * z, y * z, z], axis=-1).astype(F)


def temporal_frame(seed, px, py, front=True, t=4.0, cls=None):
    """A TW x TH frame whose pixel (x, y) lies at the world position CAM_BEFORE saw at (px[y, x], py[y, x]); normals (0, 0, 1), distance t
    (so the position radius is position_tolerance * t * 1/8)."""
    rgba, feat = frame(TW, TH, seed, cls)
    cov = feat[..., 0, 3]
    feat[..., 1, :3] = np.array([0, 0, 1], F) * cov[..., None]
    feat[..., 1, 3] = F(t) * cov
    feat[..., 2, :3] = positions_for(px, py, front) * cov[..., None]
    return rgba, feat


def previous(seed, cam, length, pos, nrm=(0, 0, 1), cls=None):
    rng = np.random.default_rng(seed)
    h, w = pos.shape[:2]
    col = rng.uniform(0.1, 2.0, (h, w, 3)).astype(F)
    lum = dr.lum(col).astype(F)
    mom = np.stack([lum, lum * lum + rng.uniform(0, 0.2, (h, w)).astype(F)], axis=-1).astype(F)
    return {"cam": dict(cam), "col": col, "lum": lum, "mom": mom, "len": np.broadcast_to(np.asarray(length, np.int32), (h, w)).copy(), "pos": np.asarray(pos, F),
            "nrm": np.broadcast_to(np.asarray(nrm, F), (h, w, 3)).copy(), "cls": np.full((h, w), COVERED, np.int32) if cls is None else np.asarray(cls, np.int32)}


def temporal():
    out = []
    ys, xs = np.mgrid[0:TH, 0:TW]
    xs, ys = xs.astype(np.float64), ys.astype(np.float64)
    grid = positions_for(xs, ys)  # the previous push saw the same plane, pixel for pixel
    sp = {"iterations": 2}

    def case(label, rgba_feat, p, prev, cam=CAM_NOW):
        out.append((label, rgba_feat[0], rgba_feat[1], p, prev, cam))

    case("no previous push", temporal_frame(900, xs, ys), tr.params(spatial=sp), None)
    for mh in (1, 2, 4):
        lens = np.tile(np.array([0, 1, 2, 3, 4, 30, 31, 32], np.int32), (TH, 2))  # 0, 1, max_history - 1, max_history among them
        p = tr.params(spatial=sp, moments_min_history=mh)
        case("identical camera, lengths, moments_min_history %d" % mh, temporal_frame(901, xs, ys), p, previous(902, CAM_NOW, lens, grid), CAM_NOW)
        case("camera, integer px, moments_min_history %d" % mh, temporal_frame(903, xs, ys), p, previous(904, CAM_BEFORE, lens, grid))
    case("max_history 4", temporal_frame(905, xs, ys), tr.params(spatial=sp, max_history=4),
         previous(906, CAM_BEFORE, np.tile(np.array([2, 3, 4, 5], np.int32), (TH, 4)), grid))
    # where the taps lie: half-way, -1.5, W + 0.5, W - 0.5 (one tap past the last column), behind the camera; a radius that takes every tap
    wide = tr.params(spatial=sp, position_tolerance=64.0)
    for label, px, py, front in (("half-way", xs + 0.5, ys + 0.5, True), ("quarter", xs - 0.25, ys + 0.75, True), ("px -1.5", xs * 0 - 1.5, ys, True),
                                 ("px -0.5", xs * 0 - 0.5, ys - 0.5, True), ("px W + 0.5", xs * 0 + TW + 0.5, ys, True),
                                 ("px W - 0.5", xs * 0 + TW - 0.5, ys + 0.5, True), ("py H - 0.5", xs + 0.5, ys * 0 + TH - 0.5, True),
                                 ("px -2", xs * 0 - 2.0, ys, True), ("px W + 1", xs * 0 + TW + 1.0, ys, True), ("behind the camera", xs, ys, False)):
        case("taps " + label, temporal_frame(910, px, py, front), wide, previous(911, CAM_BEFORE, 5, grid))
    # the position radius: t = 4, footprint 1/8, tolerance 2: r = 1.  The previous positions lie off the current ones by exactly d along x
    for d in (0.5, 1.0, 1.25):
        case("position off by %g of radius 1" % d, temporal_frame(920, xs, ys), tr.params(spatial=sp),
             previous(921, CAM_BEFORE, 5, grid + np.array([d, 0, 0], F)))
    # normal_min 0.5 against previous normals of length 0.75, 0.5, 0.25 along the current one
    for d in (0.75, 0.5, 0.25, -1.0):
        case("normal dot %g, normal_min 0.5" % d, temporal_frame(930, xs, ys), tr.params(spatial=sp, normal_min=0.5), previous(931, CAM_BEFORE, 5, grid, nrm=(0, 0, d)))
    # ... and a few ulp either side of both thresholds: r^2 = 1 against e^2 = (1 -+ 2^-22)^2 = 1 -+ 2^-21 in fp32, normal_min against 0.5 -+ 1 ulp
    for label, d in (("just inside", 1.0 - 2.0 ** -22), ("just outside", 1.0 + 2.0 ** -22)):
        case("position %s the radius" % label, temporal_frame(922, xs, ys), tr.params(spatial=sp), previous(923, CAM_BEFORE, 5, grid + np.array([d, 0, 0], F)))
    for label, d in (("just inside", np.nextafter(F(0.5), F(1))), ("just outside", np.nextafter(F(0.5), F(0)))):
        case("normal %s normal_min" % label, temporal_frame(932, xs, ys), tr.params(spatial=sp, normal_min=0.5), previous(933, CAM_BEFORE, 5, grid, nrm=(0, 0, d)))
    # the kept weight: only the tap right of x0 is of the pixel's class, its weight fx = 1e-3 -+ 2^-20
    stripes = np.where(np.arange(TW) % 2 == 1, COVERED, COVERED_EMISSIVE)[None, :] * np.ones((TH, 1), int)
    for label, fx in (("under", 1048 * 2.0 ** -20), ("over", 1049 * 2.0 ** -20)):
        even = 2 * np.floor(xs / 2)
        case("kept weight just %s kMinHistoryWeight" % label, temporal_frame(940, even + fx, ys), wide, previous(941, CAM_BEFORE, 5, grid, cls=stripes))
    # classes: history only from the pixel's own class; uncovered pixels have none
    mixed = _pattern(TW, TH, "checker", 2)
    case("classes", temporal_frame(950, xs + 0.5, ys + 0.5, cls=mixed), wide, previous(951, CAM_BEFORE, 5, grid, cls=_pattern(TW, TH, "columns", 2)))
    return out
