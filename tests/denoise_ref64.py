"""An independent float64 reference of the plain spatial filter, written from the formulas of DESIGN.md 4.10 and from nothing else: it
shares no code with tests/denoise_ref.py and is not laid out like the kernels.  Every neighbourhood is a gather through index arrays
(`_taps`); all arithmetic is float64 on the float32 inputs.  It pins the definition: the B3 taps, the class rule, the depth scale, the
squared weights on the variance, the 3 x 3 prefilter, demodulation and remodulation, and the rule for non-finite values (fmax returns the
operand that is no NaN; a tap of another class or outside the image is not read).

denoise(rgba (H, W, 4), features (H, W, 3, 4), iterations, sigma_luminance, sigma_normal, sigma_depth) -> (H, W, 4) float64.
"""
import numpy as np

ALBEDO_MIN = 0.01
DEPTH_FLOOR = 1e-3
LUM_EPS = 1e-10
LUM_WEIGHTS = np.array([0.2126, 0.7152, 0.0722])
B3 = {0: 3.0 / 8.0, 1: 1.0 / 4.0, 2: 1.0 / 16.0}
BINOMIAL = {0: 0.5, 1: 0.25}


def _taps(h, w, ox, oy):
    """Flat indices of pixel (x + ox, y + oy) for every pixel (clamped into the image) and whether that pixel exists."""
    ys, xs = np.indices((h, w))
    qx, qy = xs + ox, ys + oy
    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
    return (np.clip(qy, 0, h - 1) * w + np.clip(qx, 0, w - 1)).ravel(), inside.ravel()


def _weights(n, t, grad, same, q, ox, oy, sigma_normal, sigma_depth):
    """max(0, n_p . n_q)^sigma_n * exp(-|t_p - t_q| / (sigma_z s)), s = |grad t_p . (q - p)| + 1e-3 t_p; the exponent's argument apart."""
    with np.errstate(all="ignore"):
        wn = np.fmax(0.0, (n * n[q]).sum(axis=1)) ** sigma_normal
        if sigma_depth == 0:
            arg = np.zeros(len(t))
        else:
            s = np.abs(grad[:, 0] * ox + grad[:, 1] * oy) + DEPTH_FLOOR * t
            d = np.abs(t - t[q])
            arg = np.where(d == 0, 0.0, d / (sigma_depth * s))  # equal distances weigh 1 whatever the scale, also a scale of 0
    return wn, arg


def denoise(rgba, features, iterations=5, sigma_luminance=32.0, sigma_normal=128.0, sigma_depth=1.0, stages=None):
    rgba = np.asarray(rgba, np.float64)
    feat = np.asarray(features, np.float64)
    h, w = rgba.shape[:2]
    npx = h * w
    rgb = rgba[..., :3].reshape(npx, 3)
    albedo, coverage = feat[..., 0, :3].reshape(npx, 3), feat[..., 0, 3].ravel()
    n, t = feat[..., 1, :3].reshape(npx, 3), feat[..., 1, 3].ravel()
    emission = feat[..., 2, 3].ravel()

    # 1. prepare
    covered, emissive = coverage > 0, emission > 0
    cls = covered.astype(int) + 2 * emissive.astype(int)
    factor = np.where((covered & ~emissive)[:, None], np.fmax(albedo, ALBEDO_MIN), 1.0)
    c = rgb / factor
    lum = c @ LUM_WEIGHTS

    # 2. the gradient of t over neighbours of the same class, and the 3 x 3 variance
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
    if stages is not None:
        stages.update(c=c.reshape(h, w, 3).copy(), lum=lum.reshape(h, w).copy(), cls=cls.reshape(h, w), grad=grad.reshape(h, w, 2), var=var.reshape(h, w).copy())

    # 3. a-trous
    for i in range(iterations):
        step = 2 ** i
        g, gs = np.zeros(npx), np.zeros(npx)
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                q, inside = _taps(h, w, ox, oy)
                k = BINOMIAL[abs(ox)] * BINOMIAL[abs(oy)]
                g = g + np.where(inside, k * var[q], 0.0)
                gs = gs + np.where(inside, k, 0.0)
        with np.errstate(all="ignore"):
            lum_scale = sigma_luminance * np.sqrt(g / gs) + LUM_EPS
        sw = np.full(npx, B3[0] * B3[0])
        with np.errstate(all="ignore"):
            sc = sw[:, None] * c
            sv = sw * sw * var
        for ky in (-2, -1, 0, 1, 2):
            for kx in (-2, -1, 0, 1, 2):
                if kx == 0 and ky == 0:
                    continue
                ox, oy = kx * step, ky * step
                q, inside = _taps(h, w, ox, oy)
                same = inside & covered & (cls[q] == cls)
                wn, arg = _weights(n, t, grad, same, q, ox, oy, sigma_normal, sigma_depth)
                with np.errstate(all="ignore"):
                    if sigma_luminance != 0:
                        arg = arg + np.abs(lum - lum[q]) / lum_scale
                    wq = B3[abs(kx)] * B3[abs(ky)] * wn * np.exp(-arg)
                    sw = sw + np.where(same, wq, 0.0)
                    sc = sc + np.where(same[:, None], wq[:, None] * c[q], 0.0)
                    sv = sv + np.where(same, wq * wq * var[q], 0.0)
        with np.errstate(all="ignore"):
            c = np.where(covered[:, None], sc / sw[:, None], c)
            var = np.where(covered, sv / (sw * sw), var)
        lum = c @ LUM_WEIGHTS

    # 4. finish
    out = np.empty((h, w, 4))
    with np.errstate(all="ignore"):
        out[..., :3] = (c * factor).reshape(h, w, 3)
    out[..., 3] = rgba[..., 3]
    return out
