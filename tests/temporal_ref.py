"""numpy float32 restatement of the temporal denoiser of cpupathtrace_amd/csrc/pt_denoise.hip (pt_temporal_run) and of the
host-side camera terms pt_image.cpp hands it: the definition the GPU is checked against.  Reprojection and tap validity are only + - * /, one
square root and comparisons, all correctly rounded (the library is built with -ffp-contract=off and correctly rounded division and square
root), so the history lengths agree exactly; the filter itself is tests/denoise_ref.py's.

A push takes rgba (H, W, 4), features (H, W, 3, 4) and a camera dict (scenes.camera); the state between pushes is a TemporalState.
"""
import numpy as np

from tests import denoise_ref as dr

F = np.float32
MIN_HISTORY_WEIGHT = F(1e-3)
REPROJECT_NONE, REPROJECT_IDENTICAL, REPROJECT_CAMERA = 0, 1, 2

DEFAULTS = {"spatial": dict(dr.DEFAULTS), "alpha_color": float(F(0.2)), "alpha_moments": float(F(0.2)), "max_history": 32, "moments_min_history": 4,
            "sigma_luminance_temporal": 4.0, "normal_min": float(F(0.9)), "position_tolerance": 2.0}  # (as the library's fp32 fields read back)


def params(**kw):
    """DEFAULTS with some fields replaced ("spatial" may name only some of its own)."""
    p = {k: (dict(v) if isinstance(v, dict) else v) for k, v in DEFAULTS.items()}
    for k, v in kw.items():
        if k == "spatial":
            p["spatial"].update(v)
        else:
            p[k] = v
    return p


# ---- the camera terms (pt_api.cpp: derive_camera; pt_image.cpp: temporal_camera) ---------------------------------------------------------------------

def _dot(a, b):
    d = F(0.0)
    d = d + a[0] * b[0]
    d = d + a[1] * b[1]
    d = d + a[2] * b[2]
    return F(d)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def _normalize(a):
    inv = F(1.0) / np.sqrt(_dot(a, a))
    return (a * inv).astype(F)


def camera_basis(cam):
    """origin, forward, up, right as Camera::Camera builds them (src/host/camera.cpp), in fp32."""
    origin = np.asarray(cam["origin"], F)
    forward = (_normalize((np.asarray(cam["look_at"], F) - origin).astype(F)) * F(cam["focal_length"])).astype(F)
    half = F(cam["height"]) / F(2.0)
    up = (_normalize(np.asarray(cam["up"], F)) * half).astype(F)
    right = (_normalize(_cross(forward, up)) * (half * F(cam["aspect_ratio"]))).astype(F)
    return origin, forward, up, right


def camera_rows(cam):
    """Rows of the inverse of [forward up right] times |det|: (a, b, c) = rows . (X - origin) with X - origin = a forward + b up + c right up to
    a positive factor.  None for a degenerate basis."""
    _, f, u, r = camera_basis(cam)
    rows = np.stack([_cross(u, r), _cross(r, f), _cross(f, u)])
    det = _dot(f, rows[0])
    if not np.isfinite(det) or det == 0:
        return None
    if det < 0:
        rows = -rows
    return rows if np.isfinite(rows).all() else None


def footprint(cam, height):
    """A pixel's footprint per unit hit distance: height / (focal_length * image height)."""
    return F(cam["height"]) / (F(cam["focal_length"]) * F(height))


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def surface(features):
    """Per pixel: the mean hit position X and hit distance t of the rays that hit (features / coverage) and their mean normal scaled to unit
    length (so that a pixel on an edge matches itself); zero where no ray hit."""
    feat = np.asarray(features, F)
    cov = feat[..., 0, 3]
    covered = cov > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        X = np.where(covered[..., None], feat[..., 2, :3] / cov[..., None], F(0.0)).astype(F)
        t = np.where(covered, feat[..., 1, 3] / cov, F(0.0)).astype(F)
        v = feat[..., 1, :3]
        len2 = _dot3(v, v)
        inv = (F(1.0) / np.sqrt(len2)).astype(F)
        n = np.where((covered & (len2 > 0))[..., None], v * inv[..., None], F(0.0)).astype(F)
    return X, n, t


def project(X, cam, width, height):
    """Continuous pixel coordinates (px, py) of world points X (..., 3) in `cam` (worker.cpp's x_camera / y_camera inverted), and whether the
    point lies in front of the camera and near the image (the kernel's `found`)."""
    origin = np.asarray(cam["origin"], F)
    rows = camera_rows(cam)
    d = (X - origin).astype(F)
    a = _dot3(d, rows[0])
    b = _dot3(d, rows[1])
    c = _dot3(d, rows[2])
    front = a > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        xc = c / a
        yc = b / a
        px = ((xc * F(0.5) + F(0.5)) * F(width) - F(0.5)).astype(F)
        py = ((F(0.5) - yc * F(0.5)) * F(height) - F(0.5)).astype(F)
    found = front & (px > F(-2.0)) & (px < F(width) + F(1.0)) & (py > F(-2.0)) & (py < F(height) + F(1.0))
    return px, py, found


# ---- the temporal step (pt_temporal_accumulate_kernel) --------------------------------------------------------------------------------

class TemporalState:
    """What a pt_temporal handle keeps between pushes."""

    def __init__(self):
        self.prev = None  # dict: cam, col (H, W, 3), mom (H, W, 2), len (H, W), pos, nrm (H, W, 3), cls (H, W)

    def reset(self):
        self.prev = None


def _same_camera(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(camera_basis(a), camera_basis(b)))


def accumulate(c, l, cls, features, cam, prev, p):
    """Returns the integrated colour (H, W, 3), its luminance, the moments (H, W, 2), the history length n, and the taps the kernel used:
    (mode, x0, y0, fx, fy, valid[4]) for tests that resample with them."""
    h, w = l.shape
    X, nrm, t = surface(features)
    covered = (cls & dr.CLS_COVERED) != 0
    ys, xs = np.mgrid[0:h, 0:w]
    if prev is None:
        mode = REPROJECT_NONE
    elif _same_camera(cam, prev["cam"]):
        mode = REPROJECT_IDENTICAL
    else:
        mode = REPROJECT_CAMERA
    if mode == REPROJECT_IDENTICAL:
        px, py, found = xs.astype(F), ys.astype(F), np.ones((h, w), bool)
    elif mode == REPROJECT_CAMERA:
        px, py, found = project(X, prev["cam"], w, h)
    else:
        px, py, found = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), bool)
    found = found & covered
    px = np.where(found, px, F(0.0)).astype(F)
    py = np.where(found, py, F(0.0)).astype(F)
    x0 = np.floor(px).astype(np.int64)
    y0 = np.floor(py).astype(np.int64)
    fx = (px - x0.astype(F)).astype(F)
    fy = (py - y0.astype(F)).astype(F)
    r = F(p["position_tolerance"]) * (t * footprint(cam, h))
    r2 = r * r
    sw = np.zeros((h, w), F)
    sc = np.zeros((h, w, 3), F)
    sm = np.zeros((h, w, 2), F)
    nmax = np.zeros((h, w), np.int64)
    valid = []
    for k in range(4):
        ox, oy = k & 1, k >> 1
        wk = ((fx if ox else F(1.0) - fx) * (fy if oy else F(1.0) - fy)).astype(F)
        qx, qy = x0 + ox, y0 + oy
        ok = found & (wk > 0) & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
        if prev is not None:
            cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            ok = ok & (prev["cls"][cy, cx] == cls)
            ok = ok & (_dot3(nrm, prev["nrm"][cy, cx]) >= F(p["normal_min"]))
            e = (X - prev["pos"][cy, cx]).astype(F)
            ok = ok & (_dot3(e, e) <= r2)
            sw = np.where(ok, sw + wk, sw).astype(F)
            sc = np.where(ok[..., None], sc + wk[..., None] * prev["col"][cy, cx], sc).astype(F)
            sm = np.where(ok[..., None], sm + wk[..., None] * prev["mom"][cy, cx], sm).astype(F)
            nmax = np.where(ok, np.maximum(nmax, prev["len"][cy, cx]), nmax)
        else:
            ok = ok & False
        valid.append(ok)
    has = found & ~(sw < MIN_HISTORY_WEIGHT)
    n = np.where(has, np.minimum(1 + nmax, p["max_history"]), 1)
    n = np.where(covered, n, 0).astype(np.int32)
    blend = n > 1
    mom = np.stack([l, l * l], axis=-1).astype(F)
    col = c.copy()
    if blend.any():
        with np.errstate(divide="ignore", invalid="ignore"):
            inv_n = (F(1.0) / n.astype(F)).astype(F)
            ac = np.fmax(inv_n, F(p["alpha_color"]))[..., None]
            am = np.fmax(inv_n, F(p["alpha_moments"]))[..., None]
            hc = sc / sw[..., None]
            hm = sm / sw[..., None]
            bc = ((F(1.0) - ac) * hc + ac * c).astype(F)
            bm = ((F(1.0) - am) * hm + am * mom).astype(F)
        col = np.where(blend[..., None], bc, c).astype(F)
        mom = np.where(blend[..., None], bm, mom).astype(F)
    return col, dr.lum(col).astype(F), mom, n, (mode, x0, y0, fx, fy, valid), (X, nrm)


def push(state, rgba, features, cam, p=None):
    """One pt_temporal_denoise: returns (out (H, W, 4), history length (H, W) int32) and updates `state`."""
    p = params() if p is None else p
    sp = p["spatial"]
    rgba = np.asarray(rgba, F)
    c, l, guide, cls, factor = dr.prepare(rgba, features)
    col, l, mom, n, _, (X, nrm) = accumulate(c, l, cls, features, cam, state.prev, p)
    gx, gy = dr.gradient(guide, cls)
    var = dr.variance(l, guide, cls, gx, gy, sp["sigma_normal"], sp["sigma_depth"])
    temporal = (n >= p["moments_min_history"]) & (n >= 2)
    var = np.where(temporal, np.fmax(F(0.0), mom[..., 1] - mom[..., 0] * mom[..., 0]), var).astype(F)
    hist = col
    for i in range(sp["iterations"]):
        # each pixel's output depends on its own sigma only: the spatial and the temporal pass, chosen per pixel
        cs, ls, vs = dr.atrous(col, l, var, guide, cls, gx, gy, 1 << i, sp["sigma_luminance"], sp["sigma_normal"], sp["sigma_depth"])
        ct, lt, vt = dr.atrous(col, l, var, guide, cls, gx, gy, 1 << i, p["sigma_luminance_temporal"], sp["sigma_normal"], sp["sigma_depth"])
        col = np.where(temporal[..., None], ct, cs).astype(F)
        l = np.where(temporal, lt, ls).astype(F)
        var = np.where(temporal, vt, vs).astype(F)
        if i == 0:
            hist = col
    state.prev = {"cam": dict(cam), "col": hist, "mom": mom, "len": n, "pos": X, "nrm": nrm, "cls": cls}
    out = np.empty_like(rgba)
    out[..., :3] = col * factor
    out[..., 3] = rgba[..., 3]
    return out, n


def resample_previous(prev_out, taps):
    """prev_out (H, W, C) sampled at every pixel with the taps and renormalised weights of an accumulate() call; NaN where none was valid."""
    mode, x0, y0, fx, fy, valid = taps
    h, w = prev_out.shape[:2]
    acc = np.zeros(prev_out.shape, np.float64)
    sw = np.zeros((h, w), np.float64)
    for k in range(4):
        ox, oy = k & 1, k >> 1
        wk = ((fx if ox else 1.0 - fx) * (fy if oy else 1.0 - fy)).astype(np.float64)
        cx, cy = np.clip(x0 + ox, 0, w - 1), np.clip(y0 + oy, 0, h - 1)
        wk = np.where(valid[k], wk, 0.0)
        acc += wk[..., None] * prev_out[cy, cx]
        sw += wk
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((sw > 0)[..., None], acc / sw[..., None], np.nan)
