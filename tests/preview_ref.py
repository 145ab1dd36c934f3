"""numpy float32 restatement of the preview of an unfinished frame (pt_frame_preview): the raw preview of a parked pixel
from the CPU oracle, and the hole-aware form of the denoiser (pt_denoise.hip, kMasked), operation for operation.  The unmasked steps are
tests/denoise_ref.py's; only what the holes change is restated here.

A hole is a pixel with 0 samples (untouched, or in no tile).  Holes are never taps of another pixel, the 3x3 prefilter of the variance
included; in every a-trous pass a hole takes the normalised weighted mean of its non-hole taps of its own class (normal and depth weights on
a covered hole, the B3 weights alone on an uncovered one, no luminance term, its own weight 0), or keeps its value if their weights sum to 0.
A filled hole ends with alpha 1, one never filled with (0, 0, 0, 0).
"""
import numpy as np

from tests import denoise_ref as dr

F = np.float32
CLS_HOLE = 4


# ---- the raw preview of parked pixels, from the oracle ---------------------------------------------------------------------------------

def raw_preview(checker, cam, opt, seed, xs, ys, draws, pixel_seed, seed_to_state):
    """The raw preview of pixels (xs[i], ys[i]) after draws[i] samples: get_sample from the pixel's engine, the collected samples' rgba summed
    in fp32 in sample order, times np.float32(1) / collected ((0, 0, 0, 0) if none was collected).  pixel_seed and seed_to_state are
    pt_pixel_seed and pt_rng_seed_to_state (binding.pixel_seed, binding.seed_to_state)."""
    xs, ys, draws = np.asarray(xs), np.asarray(ys), np.asarray(draws)
    w, h = opt["image_width"], opt["image_height"]
    half = F(0.5)
    xc = F(2) * ((xs.astype(F) + half) / F(w) - half)
    yc = -(F(2) * ((ys.astype(F) + half) / F(h) - half))
    xy = np.stack([xc, yc], axis=1).astype(F)
    states = np.array([seed_to_state(pixel_seed(seed, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
    total = np.zeros((len(xs), 4), F)
    collected = np.zeros(len(xs), np.int32)
    for j in range(int(draws.max()) if len(draws) else 0):
        act = np.nonzero(draws > j)[0]
        rgba, col, st = checker.get_sample(cam, opt, xy[act], states[act])
        states[act] = st
        got = col != 0
        total[act[got]] = (total[act[got]] + rgba[got]).astype(F)
        collected[act[got]] += 1
    out = np.zeros((len(xs), 4), F)
    has = collected > 0
    out[has] = (total[has] * (F(1) / collected[has].astype(F))[:, None]).astype(F)
    return out


# ---- the hole-aware filter -----------------------------------------------------------------------------------------------------------

def prepare(rgba, features, samples):
    """dr.prepare, then a hole's colour and luminance are 0 and its class gains CLS_HOLE."""
    c, l, guide, cls, factor = dr.prepare(rgba, features)
    hole = np.asarray(samples) == 0
    c = np.where(hole[..., None], F(0.0), c).astype(F)
    l = np.where(hole, F(0.0), l).astype(F)
    cls = (cls | np.where(hole, CLS_HOLE, 0)).astype(np.int32)
    return c, l, guide, cls, factor


def variance(l, guide, cls, gx, gy, sigma_normal, sigma_depth):
    """dr.variance over the classes with the hole bit (a hole is no neighbour of another pixel); a hole's variance is 0 (not filled)."""
    v = dr.variance(l, guide, cls, gx, gy, sigma_normal, sigma_depth)
    return np.where((cls & CLS_HOLE) != 0, F(0.0), v).astype(F)


def atrous(c, l, var, guide, cls, gx, gy, step, sigma_luminance, sigma_normal, sigma_depth):
    """One pass at `step`: dr.atrous for every pixel but holes, with holes left out of the variance prefilter; then the holes' fill.
    A hole's variance becomes 1 once a pass has filled it."""
    t = guide[..., 3]
    hole = (cls & CLS_HOLE) != 0
    covered = (cls & dr.CLS_COVERED) != 0
    # the prefilter of the variance behind the luminance weight, over the 3x3 taps inside the image that are not holes
    g = np.zeros_like(var)
    gs = np.zeros_like(var)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            vq, m = dr._shift(var, dx, dy)
            cq, _ = dr._shift(cls, dx, dy, -1)
            k = np.where(m & ((cq & CLS_HOLE) == 0), dr.G3[dy + 1] * dr.G3[dx + 1], F(0.0)).astype(F)
            g = g + k * vq
            gs = gs + k
    with np.errstate(divide="ignore", invalid="ignore"):
        g = g / gs
    lum_scale = F(sigma_luminance) * np.sqrt(g) + dr.LUM_EPS
    sw = np.zeros_like(var)
    sc = np.zeros_like(c)
    sv = np.zeros_like(var)
    hw = np.zeros_like(var)  # the holes' sums
    hc = np.zeros_like(c)
    for dy in (-2, -1, 0, 1, 2):
        for dx in (-2, -1, 0, 1, 2):
            ox, oy = dx * step, dy * step
            h = dr.B3[dy + 2] * dr.B3[dx + 2]
            cq, m = dr._shift(c, ox, oy)
            lq, _ = dr._shift(l, ox, oy)
            vq, _ = dr._shift(var, ox, oy)
            if dx == 0 and dy == 0:
                w = np.full_like(var, h)
                wh = np.zeros_like(var)
            else:
                gq, _ = dr._shift(guide, ox, oy)
                clq, _ = dr._shift(cls, ox, oy, -1)
                ok = m & covered & (clq == cls)
                with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                    d = dr._depth_arg(t, gq[..., 3], gx, gy, ox, oy, sigma_depth)
                    a = d
                    if sigma_luminance != 0:
                        a = a + np.abs(l - lq) / lum_scale
                    nw = dr._normal_w(guide, gq, sigma_normal)
                    w = (h * nw) * np.exp(-a).astype(F)
                    wh = np.where(covered, (h * nw) * np.exp(-d).astype(F), h).astype(F)
                okh = m & hole & (clq == (cls & ~CLS_HOLE))
                w = np.where(ok, w, F(0.0)).astype(F)
                wh = np.where(okh, wh, F(0.0)).astype(F)
                cq = np.where((ok | okh)[..., None], cq, F(0.0))  # (a tap of weight zero by class or bounds is not read)
                vq = np.where(ok, vq, F(0.0))
            with np.errstate(invalid="ignore", over="ignore"):
                sw = sw + w
                sc = sc + w[..., None] * cq
                sv = sv + (w * w) * vq
                hw = hw + wh
                hc = hc + wh[..., None] * cq
    with np.errstate(divide="ignore", invalid="ignore"):
        c_out = (sc / sw[..., None]).astype(F)
        v_out = (sv / (sw * sw)).astype(F)
        h_out = (hc / hw[..., None]).astype(F)
    filled = hole & (hw > 0)
    plain = covered & ~hole
    c_out = np.where(plain[..., None], c_out, np.where(filled[..., None], h_out, c)).astype(F)
    v_out = np.where(plain, v_out, np.where(filled, F(1.0), var)).astype(F)
    return c_out, dr.lum(c_out).astype(F), v_out


def denoise(rgba, features, samples, iterations=5, sigma_luminance=32.0, sigma_normal=128.0, sigma_depth=1.0):
    """The hole-aware filter: (H, W, 4) float32 and the (H, W) sample counts in (0 = hole), (H, W, 4) float32 out.  Without holes it is
    dr.denoise bit for bit."""
    rgba = np.asarray(rgba, F)
    c, l, guide, cls, factor = prepare(rgba, features, samples)
    gx, gy = dr.gradient(guide, cls)
    var = variance(l, guide, cls, gx, gy, sigma_normal, sigma_depth)
    for i in range(iterations):
        c, l, var = atrous(c, l, var, guide, cls, gx, gy, 1 << i, sigma_luminance, sigma_normal, sigma_depth)
    hole = (cls & CLS_HOLE) != 0
    out = np.empty_like(rgba)
    out[..., :3] = c * factor
    out[..., 3] = np.where(hole, F(1.0), rgba[..., 3])
    out[hole & ~(var > 0)] = F(0.0)
    return out
