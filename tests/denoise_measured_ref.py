"""numpy float32 restatement of the measured form of the denoiser (pt_denoise_measured_run, cpupathtrace_amd/csrc/pt_denoise.hip; DESIGN.md
4.16), operation for operation, and of the variance map it is fed (pixel_variance, cpupathtrace_amd/csrc/pt_noise.h).  The stages the plane
does not change are tests/denoise_ref.py's and tests/preview_ref.py's; only what it changes is restated here: the variance of a rated pixel
and the luminance sigma of its a-trous weights.

plane (H, W, 4) float32: (v_r, v_g, v_b, B), the variance of the mean of every channel and the batch means behind it.  A pixel is RATED
when B >= 2 and every v_c is finite and not negative.  samples (H, W) int32 or None: 0 = a hole, as tests/preview_ref.py.
"""
import numpy as np

from tests import denoise_ref as dr
from tests import preview_ref as pr

F = np.float32
FLT_MAX = np.finfo(F).max
DEFAULTS = dict(dr.DEFAULTS, sigma_measured=16.0)


# ---- the variance map ----------------------------------------------------------------------------------------------------------------

def pixel_variance(count, m2, per_batch):
    """pixel_variance of pt_noise.h over arrays: (n, 4) float32 from the estimator's contribution_count (n,) and contribution_m2 (n, 4)."""
    count = np.asarray(count, np.int32)
    m2 = np.asarray(m2, F)
    batches = count // np.int32(per_batch)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = (batches - 1).astype(F)
        n = batches.astype(F)
        v = (m2[..., :3] / d[..., None]) / n[..., None]
        ok = (batches >= 2) & ((v >= 0) & (v <= FLT_MAX)).all(axis=-1)
    assert v.dtype == F
    out = np.zeros(m2.shape[:-1] + (4,), F)
    out[ok, :3] = v[ok]
    out[ok, 3] = n[ok]
    return out


# ---- the filter ------------------------------------------------------------------------------------------------------------------------

def rated(plane):
    """measured_variance_px of pt_denoise.hip"""
    plane = np.asarray(plane, F)
    v = plane[..., :3]
    with np.errstate(invalid="ignore"):
        return (plane[..., 3] >= F(2)) & ((v >= 0) & (v <= FLT_MAX)).all(axis=-1)


def variance(l, guide, cls, gx, gy, sigma_normal, sigma_depth, plane, features):
    """The variance stage: pr.variance, then on rated pixels that are no holes (0.2126 s_r + 0.7152 s_g + 0.0722 s_b)^2 with
    s_c = sqrt(v_c) / max(albedo_c, 0.01) on covered, non-emissive pixels and sqrt(v_c) elsewhere."""
    v = pr.variance(l, guide, cls, gx, gy, sigma_normal, sigma_depth)
    plane = np.asarray(plane, F)
    feat = np.asarray(features, F)
    use = rated(plane) & ((cls & pr.CLS_HOLE) == 0)
    demod = ((cls & dr.CLS_COVERED) != 0) & ((cls & dr.CLS_EMISSIVE) == 0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.sqrt(plane[..., :3])
        s = np.where(demod[..., None], s / np.fmax(feat[..., 0, :3], dr.ALBEDO_MIN), s).astype(F)
        sl = dr.lum(s).astype(F)
        return np.where(use, sl * sl, v).astype(F)


def atrous(c, l, var, guide, cls, gx, gy, step, sigma, sigma_normal, sigma_depth):
    """pr.atrous with a luminance sigma per pixel, `sigma` (H, W) float32: 0 turns the term off at that pixel."""
    t = guide[..., 3]
    sigma = np.asarray(sigma, F)
    hole = (cls & pr.CLS_HOLE) != 0
    covered = (cls & dr.CLS_COVERED) != 0
    g = np.zeros_like(var)
    gs = np.zeros_like(var)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            vq, m = dr._shift(var, dx, dy)
            cq, _ = dr._shift(cls, dx, dy, -1)
            k = np.where(m & ((cq & pr.CLS_HOLE) == 0), dr.G3[dy + 1] * dr.G3[dx + 1], F(0.0)).astype(F)
            with np.errstate(invalid="ignore", over="ignore"):
                g = g + k * vq
            gs = gs + k
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        g = g / gs
        lum_scale = (sigma * np.sqrt(g) + dr.LUM_EPS).astype(F)
    sw = np.zeros_like(var)
    sc = np.zeros_like(c)
    sv = np.zeros_like(var)
    hw = np.zeros_like(var)
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
                    a = np.where(sigma != 0, d + np.abs(l - lq) / lum_scale, d).astype(F)
                    nw = dr._normal_w(guide, gq, sigma_normal)
                    w = (h * nw) * np.exp(-a).astype(F)
                    wh = np.where(covered, (h * nw) * np.exp(-d).astype(F), h).astype(F)
                okh = m & hole & (clq == (cls & ~pr.CLS_HOLE))
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
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c_out = (sc / sw[..., None]).astype(F)
        v_out = (sv / (sw * sw)).astype(F)
        h_out = (hc / hw[..., None]).astype(F)
    filled = hole & (hw > 0)
    plain = covered & ~hole
    c_out = np.where(plain[..., None], c_out, np.where(filled[..., None], h_out, c)).astype(F)
    v_out = np.where(plain, v_out, np.where(filled, F(1.0), var)).astype(F)
    return c_out, dr.lum(c_out).astype(F), v_out


def pixel_sigma(plane, sigma_luminance, sigma_measured):
    return np.where(rated(plane), F(sigma_measured), F(sigma_luminance)).astype(F)


def denoise(rgba, features, plane, samples=None, iterations=5, sigma_luminance=32.0, sigma_normal=128.0, sigma_depth=1.0, sigma_measured=16.0, stages=None):
    """The whole measured form: (H, W, 4) float32 out.  samples None: the plain filter's stages (no holes)."""
    rgba = np.asarray(rgba, F)
    masked = samples is not None
    s = np.asarray(samples) if masked else np.ones(rgba.shape[:2], np.int32)
    c, l, guide, cls, factor = pr.prepare(rgba, features, s)
    gx, gy = dr.gradient(guide, cls)
    var = variance(l, guide, cls, gx, gy, sigma_normal, sigma_depth, plane, features)
    if stages is not None:
        stages.update(c=c, l=l, guide=guide, cls=cls, gx=gx, gy=gy, var=var)
    sigma = pixel_sigma(plane, sigma_luminance, sigma_measured)
    for i in range(iterations):
        c, l, var = atrous(c, l, var, guide, cls, gx, gy, 1 << i, sigma, sigma_normal, sigma_depth)
    hole = (cls & pr.CLS_HOLE) != 0
    out = np.empty_like(rgba)
    with np.errstate(invalid="ignore", over="ignore"):
        out[..., :3] = c * factor
    out[..., 3] = np.where(hole, F(1.0), rgba[..., 3])
    out[hole & ~(var > 0)] = F(0.0)
    return out
