"""Meshes, shapes and the bending-card scenario shared by tests/test_motion_shapes_cpu.py and tests/test_gpu_motion_shapes.py
(include/pt_motion_shapes.h).  numpy only."""
import math

import numpy as np

from cpupathtrace_amd import scenes
from tests import motion_shapes_ref as msr
from tests import temporal_ref

F = np.float32


def grid(nx, ny, lo, hi, z=None):
    """An nx x ny-quad grid over [lo, hi] in x and y, two triangles per quad, facing -z: (vertices ((nx+1)(ny+1), 3), faces (2 nx ny, 3))."""
    xs, ys = np.linspace(lo[0], hi[0], nx + 1), np.linspace(lo[1], hi[1], ny + 1)
    gx, gy = np.meshgrid(xs, ys)
    gz = np.zeros_like(gx) if z is None else z(gx, gy)
    vertices = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(F)
    faces = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            faces += [[a, c, b], [a, d, c]]
    return vertices, np.array(faces, np.int32)


def patch():
    """The 6 x 6-quad smooth patch: 49 vertices, 72 faces, gently bumped."""
    return grid(6, 6, (-0.5, -0.5), (0.5, 0.5), lambda x, y: 0.06 * np.sin(3.0 * x) * np.cos(2.0 * y))


def patch_bent(amount):
    v, _ = patch()
    out = v.copy()
    out[:, 2] += F(amount) * (v[:, 0] * v[:, 0] - v[:, 1]).astype(F)
    out[:, 0] += F(0.3 * amount) * v[:, 1]
    return out.astype(F)


def flat8():
    """A 2 x 2-quad flat mesh (8 faces) with two degenerate faces spliced in at 2 and 7, so that a triangle's index is not its face's:
    (0, 0, 1), which no shape revives, and (9, 10, 11), three extra vertices that coincide at rest.  12 vertices, 10 faces."""
    v, f = grid(2, 2, (-0.5, -0.5), (0.5, 0.5))
    vertices = np.concatenate([v, np.tile(np.array([[0.1, 0.1, -0.05]], F), (3, 1))]).astype(F)
    faces = np.concatenate([f[:2], [[0, 0, 1]], f[2:6], [[9, 11, 10]], f[6:]]).astype(np.int32)
    return vertices, faces


def flat8_revived():
    """flat8's vertices with the three coincident ones apart: face 7 survives, in front of the grid, and the grid itself is sheared."""
    v, _ = flat8()
    out = v.copy()
    out[:9, 0] += F(0.08) * v[:9, 1]
    out[9:] = np.array([[-0.35, -0.3, -0.12], [0.4, -0.25, -0.12], [0.0, 0.4, -0.1]], F)
    return out


def place(x, y, z, scale, degrees=0.0):
    a = math.radians(degrees)
    m = np.eye(4, dtype=F)
    m[0, 0] = m[1, 1] = scale * math.cos(a)
    m[0, 1], m[1, 0] = -scale * math.sin(a), scale * math.sin(a)
    m[2, 2] = scale
    m[:3, 3] = (x, y, z)
    return m


def assemble(matrix, vertices, faces):
    """The assembler's flat triangles of one instance in numpy (kb_transform, kb_face_keep, kb_expand): (pos (n, 9), nrm (n, 9))."""
    tv = msr.transform(matrix, vertices)
    f = np.asarray(faces).reshape(-1, 3)[msr.kept_faces(matrix, vertices, faces)]
    a, b, c = tv[f[:, 0]], tv[f[:, 1]], tv[f[:, 2]]
    cr = msr._cross((b - a).astype(F), (c - a).astype(F))
    inv = (F(1.0) / np.sqrt(msr._dot_from_zero(cr, cr))).astype(F)
    n = (cr * inv[:, None]).astype(F)
    return np.concatenate([a, b, c], axis=1).astype(F), np.concatenate([n, n, n], axis=1).astype(F)


# ---- the bending card (test_a_sliding_card_keeps_its_history's camera and box) -------------------------------------------------------------

CARD_W, CARD_H = 64, 48
CARD_CAMERA = scenes.camera((0.0, 0.0, -0.9), (0.0, 0.0, 1.0), (0, 1, 0), 0.6, 1.0, -CARD_W / float(CARD_H))
CARD_AT = place(-0.05, 0.02, 0.5, 1.0)
CARD_LO, CARD_HI = (-0.31, -0.27), (0.33, 0.29)


def card():
    """An 8 x 8-quad card, flat."""
    return grid(8, 8, CARD_LO, CARD_HI)


def card_tolerance():
    """The push's position tolerance at the card: position_tolerance footprints at its distance of 1.4 from the camera."""
    return float(temporal_ref.params()["position_tolerance"]) * 1.4 * float(temporal_ref.footprint(CARD_CAMERA, CARD_H))


def card_bowed():
    """The card bowed toward the camera (-z) by 6 tolerances at its centre, falling to 0 at its border: more than one tolerance over
    well above half of its area."""
    v, _ = card()
    cx, cy = 0.5 * (CARD_LO[0] + CARD_HI[0]), 0.5 * (CARD_LO[1] + CARD_HI[1])
    hx, hy = 0.5 * (CARD_HI[0] - CARD_LO[0]), 0.5 * (CARD_HI[1] - CARD_LO[1])
    u, w = (v[:, 0] - cx) / hx, (v[:, 1] - cy) / hy
    out = v.copy()
    out[:, 2] = (-6.0 * card_tolerance() * (1.0 - u ** 2) * (1.0 - w ** 2)).astype(F)
    return out


def dilate(mask):
    out = mask.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            shifted = np.zeros_like(mask)
            ys, xs = slice(max(dy, 0), mask.shape[0] + min(dy, 0)), slice(max(dx, 0), mask.shape[1] + min(dx, 0))
            yd, xd = slice(max(-dy, 0), mask.shape[0] + min(-dy, 0)), slice(max(-dx, 0), mask.shape[1] + min(-dx, 0))
            shifted[yd, xd] = mask[ys, xs]
            out |= shifted
    return out


def check_card(f0, on0, f1, m1, n0, n_marked, n_plain, w, h):
    """The conditions of the bending-card test on: the features of both frames, a motion of frame 0 that marks the card's rays
    (motion[0].w), the marked motion of frame 1, and the history lengths of the first push, of the second with the marked motion and of
    the second with motion=None.  Silhouette, seam and tie pixels are left out exactly as test_a_sliding_card_keeps_its_history does."""
    whole = (f0[..., 0, 3] == 1) & (f1[..., 0, 3] == 1)
    assert whole.mean() >= 0.97
    full0, full1, any0, any1 = on0[..., 0, 3] == 1, m1[..., 0, 3] == 1, on0[..., 0, 3] > 0, m1[..., 0, 3] > 0
    near = dilate(any0 & ~full0) | dilate(any1 & ~full1)
    assert full1.sum() >= 100 and near.mean() < 0.15, (int(full1.sum()), float(near.mean()))
    assert (n0 == 1).all()
    card_px = full0 & full1 & ~near & whole
    ties = ~any0 & ~any1 & ~(f0 == f1).all(axis=(-1, -2))
    assert ties.sum() <= 0.01 * w * h
    wall = ~any0 & ~any1 & ~near & whole & ~ties
    lost = (n_plain[card_px] == 1).mean()
    print("%d card pixels, %d wall, %d near the silhouette (%.1f %%); without the marked motion %.1f %% of the card pixels lose their history" % (
        card_px.sum(), wall.sum(), near.sum(), 100 * near.mean(), 100 * lost))
    assert card_px.sum() >= 50 and (n_marked[card_px] == 2).all(), np.unique(n_marked[card_px], return_counts=True)
    assert lost >= 0.5, lost
    assert wall.sum() >= 0.5 * w * h and (n_marked[wall] == 2).all() and (n_plain[wall] == 2).all()
