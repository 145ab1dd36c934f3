"""numpy float32 restatement of the motion form of the temporal denoiser (pt_denoise.hip: pt_temporal_run_motion; include/pt_motion.h,
DESIGN.md 4.11.1): tests/temporal_ref.py's push with the frame's motion.  What is reprojected and compared with the taps is where the
pixel's surface was at the previous pose (Xr, nr); what is stored for the next push stays the current position and normal.  With
motion None, or a motion in which nothing moved, every operation is temporal_ref.push's: the same bits (tests/test_motion_cpu.py).
"""
import numpy as np

from tests import denoise_ref as dr
from tests import temporal_ref as tr

F = np.float32


def static_motion(features):
    """The motion of a frame in which nothing moved: the features' position and normal, both w = 0."""
    feat = np.asarray(features, F)
    m = np.zeros(feat.shape[:2] + (2, 4), F)
    m[..., 0, :3] = feat[..., 2, :3]
    m[..., 1, :3] = feat[..., 1, :3]
    return m


def previous_surface(features, motion):
    """Per pixel: Xr = motion[0].xyz / coverage and nr = motion[1].xyz at unit length (zero where no ray hit), as tr.surface forms X and n."""
    feat, mot = np.asarray(features, F), np.asarray(motion, F)
    cov = feat[..., 0, 3]
    covered = cov > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        Xr = np.where(covered[..., None], mot[..., 0, :3] / cov[..., None], F(0.0)).astype(F)
        v = mot[..., 1, :3]
        len2 = tr._dot3(v, v)
        inv = (F(1.0) / np.sqrt(len2)).astype(F)
        nr = np.where((covered & (len2 > 0))[..., None], v * inv[..., None], F(0.0)).astype(F)
    return Xr, nr


def accumulate(c, l, cls, features, motion, cam, prev, p):
    """tr.accumulate with motion (None: the plain step): the same returns."""
    h, w = l.shape
    X, nrm, t = tr.surface(features)
    covered = (cls & dr.CLS_COVERED) != 0
    ys, xs = np.mgrid[0:h, 0:w]
    if prev is None:
        mode = tr.REPROJECT_NONE
    elif tr._same_camera(cam, prev["cam"]):
        mode = tr.REPROJECT_IDENTICAL
    else:
        mode = tr.REPROJECT_CAMERA
    own = np.full((h, w), mode == tr.REPROJECT_IDENTICAL)
    proj = np.full((h, w), mode == tr.REPROJECT_CAMERA)
    Xr, nr = X, nrm
    if motion is not None:
        mot = np.asarray(motion, F)
        Xr, nr = previous_surface(features, mot)
        had = ~(mot[..., 1, 3] > 0)
        still = mot[..., 0, 3] == 0
        proj = had & (proj | (own & ~still))
        own = had & own & still
    px, py, found = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), bool)
    if proj.any():
        with np.errstate(invalid="ignore", over="ignore"):
            qx, qy, qf = tr.project(Xr, prev["cam"], w, h)
        px, py, found = np.where(proj, qx, px), np.where(proj, qy, py), proj & qf
    px = np.where(own, xs.astype(F), px).astype(F)
    py = np.where(own, ys.astype(F), py).astype(F)
    found = (found | own) & covered
    px = np.where(found, px, F(0.0)).astype(F)
    py = np.where(found, py, F(0.0)).astype(F)
    x0 = np.floor(px).astype(np.int64)
    y0 = np.floor(py).astype(np.int64)
    fx = (px - x0.astype(F)).astype(F)
    fy = (py - y0.astype(F)).astype(F)
    r = F(p["position_tolerance"]) * (t * tr.footprint(cam, h))
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
            ok = ok & (tr._dot3(nr, prev["nrm"][cy, cx]) >= F(p["normal_min"]))
            e = (Xr - prev["pos"][cy, cx]).astype(F)
            ok = ok & (tr._dot3(e, e) <= r2)
            sw = np.where(ok, sw + wk, sw).astype(F)
            sc = np.where(ok[..., None], sc + wk[..., None] * prev["col"][cy, cx], sc).astype(F)
            sm = np.where(ok[..., None], sm + wk[..., None] * prev["mom"][cy, cx], sm).astype(F)
            nmax = np.where(ok, np.maximum(nmax, prev["len"][cy, cx]), nmax)
        else:
            ok = ok & False
        valid.append(ok)
    has = found & ~(sw < tr.MIN_HISTORY_WEIGHT)
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


def push(state, rgba, features, motion, cam, p=None):
    """One pt_temporal_denoise_motion: returns (out (H, W, 4), history length (H, W) int32) and updates `state` (a tr.TemporalState)."""
    p = tr.params() if p is None else p
    sp = p["spatial"]
    rgba = np.asarray(rgba, F)
    c, l, guide, cls, factor = dr.prepare(rgba, features)
    col, l, mom, n, _, (X, nrm) = accumulate(c, l, cls, features, motion, cam, state.prev, p)
    gx, gy = dr.gradient(guide, cls)
    var = dr.variance(l, guide, cls, gx, gy, sp["sigma_normal"], sp["sigma_depth"])
    temporal = (n >= p["moments_min_history"]) & (n >= 2)
    var = np.where(temporal, np.fmax(F(0.0), mom[..., 1] - mom[..., 0] * mom[..., 0]), var).astype(F)
    hist = col
    for i in range(sp["iterations"]):
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
