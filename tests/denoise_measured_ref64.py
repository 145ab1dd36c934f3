"""An independent float64 reference of the measured form of the denoiser, holes included, written from the
formulas and laid out like tests/denoise_ref64.py, whose tap and weight helpers it uses: gathers through index arrays, all arithmetic float64
on the float32 inputs.  It pins what the plane changes -- which pixels are rated, the fully correlated luminance variance over the albedo
floor, the luminance sigma per pixel -- and what it must not change.

denoise(rgba (H, W, 4), features (H, W, 3, 4), plane (H, W, 4), samples (H, W) or None, ...) -> (H, W, 4) float64.
"""
import numpy as np

from tests.denoise_ref64 import ALBEDO_MIN, B3, BINOMIAL, LUM_EPS, LUM_WEIGHTS, _taps, _weights

HOLE = 4


def rated(plane):
    """B >= 2 and every v_c a finite fp32 number that is not negative (judged on the fp32 plane)."""
    plane = np.asarray(plane, np.float32)
    with np.errstate(invalid="ignore"):
        return ((plane[..., 3] >= 2) & np.isfinite(plane[..., :3]).all(axis=-1) & (plane[..., :3] >= 0).all(axis=-1)).ravel()


def denoise(rgba, features, plane, samples=None, iterations=5, sigma_luminance=32.0, sigma_normal=128.0, sigma_depth=1.0, sigma_measured=16.0, stages=None):
    is_rated = rated(plane)
    rgba = np.asarray(rgba, np.float64)
    feat = np.asarray(features, np.float64)
    v_mean = np.asarray(plane, np.float64)[..., :3]
    h, w = rgba.shape[:2]
    npx = h * w
    rgb = rgba[..., :3].reshape(npx, 3)
    albedo, coverage = feat[..., 0, :3].reshape(npx, 3), feat[..., 0, 3].ravel()
    n, t = feat[..., 1, :3].reshape(npx, 3), feat[..., 1, 3].ravel()
    emission = feat[..., 2, 3].ravel()
    hole = np.zeros(npx, bool) if samples is None else (np.asarray(samples).ravel() == 0)

    # 1. prepare: a hole is a class of its own and black
    covered, emissive = coverage > 0, emission > 0
    cls = covered.astype(int) + 2 * emissive.astype(int) + HOLE * hole.astype(int)
    factor = np.where((covered & ~emissive)[:, None], np.fmax(albedo, ALBEDO_MIN), 1.0)
    with np.errstate(all="ignore"):
        c = np.where(hole[:, None], 0.0, rgb / factor)
    lum = c @ LUM_WEIGHTS

    # 2. the gradient, the 3 x 3 variance, and the measured variance where the plane rates the pixel
    grad = np.zeros((npx, 2))
    for axis, (dx, dy) in enumerate(((1, 0), (0, 1))):
        qn, mn = _taps(h, w, dx, dy)
        qp, mp = _taps(h, w, -dx, -dy)
        nxt, prv = mn & (cls[qn] == cls), mp & (cls[qp] == cls)
        with np.errstate(all="ignore"):
            both, fwd, back = (t[qn] - t[qp]) / 2, t[qn] - t, t - t[qp]
        grad[:, axis] = np.where(covered, np.where(nxt & prv, both, np.where(nxt, fwd, np.where(prv, back, 0.0))), 0.0)
    sw, m1, m2 = np.ones(npx), lum.copy(), lum * lum
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            if ox == 0 and oy == 0:
                continue
            q, inside = _taps(h, w, ox, oy)
            same = inside & covered & (cls[q] == cls)
            wn, arg = _weights(n, t, grad, same, q, ox, oy, sigma_normal, sigma_depth)
            with np.errstate(all="ignore"):
                wq = wn * np.exp(-arg)
                lq = lum[q]
                sw = sw + np.where(same, wq, 0.0)
                m1 = m1 + np.where(same, wq * lq, 0.0)
                m2 = m2 + np.where(same, wq * lq * lq, 0.0)
    with np.errstate(all="ignore"):
        var = np.fmax(0.0, m2 / sw - (m1 / sw) ** 2)
        # the standard deviation of every channel's mean in the unit of c, the channels fully correlated
        sd = (np.sqrt(v_mean.reshape(npx, 3)) / factor) @ LUM_WEIGHTS
    var = np.where(is_rated, sd * sd, var)
    var = np.where(hole, 0.0, var)
    sigma_l = np.where(is_rated, float(sigma_measured), float(sigma_luminance))
    if stages is not None:
        stages.update(c=c.reshape(h, w, 3).copy(), lum=lum.reshape(h, w).copy(), cls=cls.reshape(h, w), grad=grad.reshape(h, w, 2), var=var.reshape(h, w).copy())

    # 3. a-trous: holes are no taps (not of the prefilter either) and are filled from the taps of their class that are not holes
    for i in range(iterations):
        step = 2 ** i
        g, gs = np.zeros(npx), np.zeros(npx)
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                q, inside = _taps(h, w, ox, oy)
                use = inside & ~hole[q]
                k = BINOMIAL[abs(ox)] * BINOMIAL[abs(oy)]
                with np.errstate(all="ignore"):
                    g = g + np.where(use, k * var[q], 0.0)
                gs = gs + np.where(use, k, 0.0)
        with np.errstate(all="ignore"):
            lum_scale = sigma_l * np.sqrt(g / gs) + LUM_EPS
        sw = np.full(npx, B3[0] * B3[0])
        with np.errstate(all="ignore"):
            sc = sw[:, None] * c
            sv = sw * sw * var
        fw, fc = np.zeros(npx), np.zeros((npx, 3))
        for ky in (-2, -1, 0, 1, 2):
            for kx in (-2, -1, 0, 1, 2):
                if kx == 0 and ky == 0:
                    continue
                ox, oy = kx * step, ky * step
                q, inside = _taps(h, w, ox, oy)
                same = inside & covered & (cls[q] == cls)
                fill = inside & hole & (cls[q] == cls - HOLE)
                wn, arg = _weights(n, t, grad, same, q, ox, oy, sigma_normal, sigma_depth)
                b = B3[abs(kx)] * B3[abs(ky)]
                with np.errstate(all="ignore"):
                    wf = np.where(covered, b * wn * np.exp(-arg), b)
                    arg = np.where(sigma_l != 0, arg + np.abs(lum - lum[q]) / lum_scale, arg)
                    wq = b * wn * np.exp(-arg)
                    sw = sw + np.where(same, wq, 0.0)
                    sc = sc + np.where(same[:, None], wq[:, None] * c[q], 0.0)
                    sv = sv + np.where(same, wq * wq * var[q], 0.0)
                    fw = fw + np.where(fill, wf, 0.0)
                    fc = fc + np.where(fill[:, None], wf[:, None] * c[q], 0.0)
        plain, filled = covered & ~hole, hole & (fw > 0)
        with np.errstate(all="ignore"):
            c = np.where(plain[:, None], sc / sw[:, None], np.where(filled[:, None], fc / fw[:, None], c))
            var = np.where(plain, sv / (sw * sw), np.where(filled, 1.0, var))
        lum = c @ LUM_WEIGHTS

    # 4. finish
    out = np.empty((h, w, 4))
    with np.errstate(all="ignore"):
        out[..., :3] = (c * factor).reshape(h, w, 3)
    out[..., 3] = np.where(hole, 1.0, rgba[..., 3].ravel()).reshape(h, w)
    out[(hole & ~(var > 0)).reshape(h, w)] = 0.0
    return out
