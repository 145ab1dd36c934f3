"""Deterministic synthetic frames for the measured form of the denoiser (pt_denoise_measured_run): the frames of
tests/denoise_cases.py with a plane of measured variances.  Each family returns a list of cases

    (label, rgba (H, W, 4), features (H, W, 3, 4), plane (H, W, 4), samples (H, W) int32 or None, params)

from fixed seeds; params are tests/denoise_measured_ref.py's DEFAULTS with changes.  tests/test_denoise_measured_cpu.py checks the fp32
restatement on them against the float64 reference (tests/denoise_measured_ref64.py); tests/test_gpu_denoise_measured.py runs them on the
device through tests/denoise_measured_probe.py.  Sizes are width x height.
"""
import numpy as np

from tests import denoise_cases as dc
from tests import denoise_measured_ref as mr

F = np.float32
SIZES = [(1, 1), (1, 40), (40, 1), (3, 3), (17, 33), (48, 40), (70, 70)]  # (five passes, the default, at every size)
DENORMAL = F(1e-40)


def P(**kw):
    return dict(mr.DEFAULTS, **kw)


def plane_for(rgba, seed, batches=None, scale=0.5):
    """A plausible plane: the standard deviation of every channel's mean is `scale` (0.5 .. 1.5 of it, per pixel) of the channel's value,
    B = 2 .. 9 batch means (or `batches`)."""
    rng = np.random.default_rng(seed)
    h, w = rgba.shape[:2]
    sd = (np.abs(rgba[..., :3]) * F(scale) * rng.uniform(0.5, 1.5, (h, w, 1))).astype(F)
    plane = np.empty((h, w, 4), F)
    plane[..., :3] = sd * sd
    plane[..., 3] = rng.integers(2, 10, (h, w)).astype(F) if batches is None else np.broadcast_to(np.asarray(batches, F), (h, w))
    return plane


def unrate(plane, where):
    """The plane with the pixels of `where` as pt_frame_get_variance writes an unrated pixel: (0, 0, 0, 0)."""
    out = plane.copy()
    out[where] = F(0)
    return out


def pattern(w, h, kind, period):
    ys, xs = np.mgrid[0:h, 0:w]
    return ((xs // period + ys // period) % 2 == 0) if kind == "checker" else ((xs // period) % 2 == 0)


def unrated():
    """B = 0 everywhere: the existing filter, plain and with holes."""
    out = []
    for i, (w, h) in enumerate(SIZES):
        rgba, feat = dc.frame(w, h, 1100 + i, dc._pattern(w, h, "checker", 4) if i % 2 else None)
        rng = np.random.default_rng(1150 + i)
        out.append(("%dx%d" % (w, h), rgba, feat, np.zeros((h, w, 4), F), None, P()))
        out.append(("%dx%d, holes" % (w, h), rgba, feat, np.zeros((h, w, 4), F), rng.integers(0, 3, (h, w)).astype(np.int32), P()))
    # v_c set but B below 2: unrated all the same
    rgba, feat = dc.frame(33, 31, 1160)
    out.append(("B = 1 everywhere", rgba, feat, plane_for(rgba, 1161, batches=1), None, P()))
    return out


def rated_all():
    """B >= 2 everywhere, every size."""
    out = []
    for i, (w, h) in enumerate(SIZES):
        rgba, feat = dc.frame(w, h, 1200 + i)
        out.append(("%dx%d" % (w, h), rgba, feat, plane_for(rgba, 1250 + i), None, P()))
    return out


def patterns():
    """Checkerboards and columns of rated and unrated pixels."""
    out = []
    w, h = 33, 31
    for kind in ("checker", "columns"):
        for period in (1, 2, 4):
            rgba, feat = dc.frame(w, h, 1300 + period)
            out.append(("%s/%d" % (kind, period), rgba, feat, unrate(plane_for(rgba, 1310 + period), pattern(w, h, kind, period)), None, P(iterations=3)))
    return out


def borders():
    """Rated pixels either side of class borders and next to holes."""
    out = []
    w, h = 33, 31
    ys, xs = np.mgrid[0:h, 0:w]
    cls = np.full((h, w), dc.COVERED)
    cls[:, 20:] = dc.COVERED_EMISSIVE
    cls[24:, :] = dc.UNCOVERED
    cls[24:, 26:] = dc.EMISSIVE
    rgba, feat = dc.frame(w, h, 1400, cls)
    plane = plane_for(rgba, 1401)
    out.append(("all four classes, all rated", rgba, feat, plane, None, P()))
    near = (np.abs(xs - 20) <= 1) | (np.abs(ys - 24) <= 1)
    out.append(("rated along the borders only", rgba, feat, unrate(plane, ~near), None, P()))
    out.append(("unrated along the borders only", rgba, feat, unrate(plane, near), None, P()))
    rng = np.random.default_rng(1402)
    s = rng.integers(1, 9, (h, w)).astype(np.int32)
    s[5:8, 5:8] = 0
    s[10, 19:22] = 0
    s[22:26, 10] = 0
    s[rng.random((h, w)) < 0.1] = 0
    out.append(("holes, all rated (the holes too)", rgba, feat, plane, s, P()))
    out.append(("holes, the rest rated", rgba, feat, unrate(plane, s == 0), s, P()))
    ring = np.zeros((h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ring |= np.roll(np.roll(s == 0, dy, 0), dx, 1)
    out.append(("holes, rated next to them only", rgba, feat, unrate(plane, ~ring), s, P()))
    return out


def values():
    """v_c of 0, denormal, 1e-30 and 1e30; albedo 0, 0.0099, 0.01 and 1; B = 1 and B = 2."""
    out = []
    w, h = 33, 31
    ys, xs = np.mgrid[0:h, 0:w]
    sel = pattern(w, h, "checker", 2)
    for i, (name, v) in enumerate((("0", F(0)), ("denormal", DENORMAL), ("1e-30", F(1e-30)), ("1e30", F(1e30)))):
        rgba, feat = dc.frame(w, h, 1500 + i)
        plane = plane_for(rgba, 1510 + i)
        plane[sel, :3] = v
        out.append(("v %s in places" % name, rgba, feat, plane, None, P(iterations=3)))
        plane = plane.copy()
        plane[..., :3] = v
        out.append(("v %s everywhere" % name, rgba, feat, plane, None, P(iterations=3)))
    for i, a in enumerate((0.0, 0.0099, 0.01, 1.0)):
        amap = np.where(((xs // 2 + ys) % 2 == 0)[..., None], F(a), F(0.5)).astype(F) * np.ones(3, F)
        rgba, feat = dc.frame(w, h, 1520 + i, albedo=amap)
        out.append(("albedo %g" % a, rgba, feat, plane_for(rgba, 1530 + i), None, P(iterations=3)))
    rgba, feat = dc.frame(w, h, 1540)
    out.append(("B = 1 and B = 2", rgba, feat, plane_for(rgba, 1541, batches=np.where(sel, F(1), F(2))), None, P(iterations=3)))
    out.append(("B = 2 and B = 1e6", rgba, feat, plane_for(rgba, 1542, batches=np.where(sel, F(2), F(1e6))), None, P(iterations=3)))
    return out


NONFINITE_AT = [(10, 10), (10, 19), (10, 21), (26, 5), (15, 30)]


def nonfinite():
    """NaN, negative and infinite v_c (and B): the pixel falls back to the spatial estimate."""
    out = []
    w, h = 33, 31
    cls = np.full((h, w), dc.COVERED)
    cls[:, 20:] = dc.COVERED_EMISSIVE
    cls[24:, :] = dc.UNCOVERED
    for i, (name, v) in enumerate((("nan", np.nan), ("negative", -1e-3), ("-0", -0.0), ("inf", np.inf), ("-inf", -np.inf))):
        rgba, feat = dc.frame(w, h, 1600, cls)
        plane = plane_for(rgba, 1601)
        for k, (y, x) in enumerate(NONFINITE_AT):
            plane[y, x, k % 3] = F(v)
        out.append(("v " + name, rgba, feat, plane, None, P(iterations=2)))
    for name, v in (("nan", np.nan), ("inf", np.inf), ("-2", -2.0)):
        rgba, feat = dc.frame(w, h, 1610, cls)
        plane = plane_for(rgba, 1611)
        for y, x in NONFINITE_AT:
            plane[y, x, 3] = F(v)
        out.append(("B " + name, rgba, feat, plane, None, P(iterations=2)))
    return out


def parameters():
    out = []
    w, h = 33, 31
    cls = np.where(dc._pattern(w, h, "checker", 4) == dc.UNCOVERED, dc.COVERED, dc._pattern(w, h, "checker", 4))
    rgba, feat = dc.frame(w, h, 1700, cls)
    plane = unrate(plane_for(rgba, 1701), pattern(w, h, "columns", 4))
    for sm in (0.0, 1.0, 32.0):
        out.append(("sigma_measured %g" % sm, rgba, feat, plane, None, P(iterations=3, sigma_measured=sm)))
    out.append(("sigma_luminance 0", rgba, feat, plane, None, P(iterations=3, sigma_luminance=0.0)))
    out.append(("both luminance sigmas 0", rgba, feat, plane, None, P(iterations=3, sigma_luminance=0.0, sigma_measured=0.0)))
    for it in (0, 1):
        out.append(("iterations %d" % it, rgba, feat, plane, None, P(iterations=it)))
    return out


FAMILIES = {"unrated": unrated, "rated": rated_all, "patterns": patterns, "borders": borders, "values": values, "nonfinite": nonfinite,
            "parameters": parameters}

# E(restatement) = tests/denoise_cases.py's error(): max |x - ref64| / (|ref64| + 1e-3 mean |ref64|) over rgb, the largest of each family's
# cases: tests/denoise_measured_ref.py against tests/denoise_measured_ref64.py on the CPU (tests/test_denoise_measured_cpu.py prints them),
# rounded up to two digits, over the pixels of ref64_mask below.  The device is held to 4 x these (tests/test_gpu_denoise_measured.py).
E_RESTATEMENT = {"unrated": 3.6e-6, "rated": 4.7e-7, "patterns": 4.4e-7, "borders": 3.8e-7, "values": 6.3e-7, "nonfinite": 5.4e-7, "parameters": 4.1e-7}


def ref64_mask(samples, shape):
    """Where ref64 can stand for the fp32 definition: everywhere but on holes.  A hole's fill is a ratio of sums of weights without the
    centre tap's 9/64 in them; behind a depth term of exp(-100) they lie in fp32's denormal range or below it (the hole then keeps its
    value in fp32 and is filled in fp64), so there the two are different filters.  Holes are taps of no other pixel, so leaving them out
    hides nothing about the rest; they are held to the fp32 restatement like every pixel."""
    return np.ones(shape, bool) if samples is None else np.asarray(samples) != 0


def preservation_interior():
    """The pixels of the preservation frame more than three columns right of the border between its halves: the blur of the border
    pixels (their prefiltered variance holds the left half's) reaches no farther in five passes (tests/test_denoise_measured_cpu.py)."""
    ys, xs = np.mgrid[0:40, 0:48]
    return xs >= 24 + 4


# ---- the preservation case ------------------------------------------------------------------------------------------------------------

def preservation():
    """A 48 x 40 frame on one plane: the left half log-normal noise with a large measured variance, the right half a fine luminance texture
    of period 2 (columns of 0.4 and 0.8) with a measured variance of 1e-12.  Returns (rgba, features, plane, right), `right` the mask of
    the right half's pixels that no tap of the left half reaches in one pass less than the filter runs."""
    w, h = 48, 40
    rgba, feat = dc.frame(w, h, 1800, albedo=0.5)
    ys, xs = np.mgrid[0:h, 0:w]
    right = xs >= w // 2
    tex = np.where(xs % 2 == 0, F(0.4), F(0.8)).astype(F)
    rgba[right, :3] = tex[right][:, None]
    plane = np.empty((h, w, 4), F)
    plane[..., :3] = np.where(right[..., None], F(1e-12), (rgba[..., :3] * F(0.5)) ** 2).astype(F)
    plane[..., 3] = F(8)
    return rgba, feat, plane, right
