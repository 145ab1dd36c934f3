"""Indexed meshes and transforms for the mesh-assembly tests (include/pt_mesh.h): the smallest shapes at which the device's transform,
face rejection, order-preserving compaction and serial normal sums can go wrong.  Everything is deterministic from a seed.

MESHES     name -> (vertices (n, 3) float32, faces (m, 3) int32).  Faces may name indices < 0 and >= n; one vertex may have a NaN x.
TRANSFORMS name -> 4 x 4 float32 matrix (rows, as mat4).
obj_text   the mesh as OBJ text for the host loaders: %.9g numbers (they round-trip float32 exactly), all v lines before all f lines,
           a NaN x written as a lone '-' (which the reader turns into NaN).
"""
import ctypes as C

import numpy as np

F = np.float32

GUARD_ROWS = 16  # rows of 0xA5 bytes on either side of an output array


def _distinct_triples(rng, n_vertices, n_faces):
    faces = np.empty((n_faces, 3), np.int32)
    for i in range(n_faces):
        faces[i] = rng.choice(n_vertices, 3, replace=False)
    return faces


def sized(n_faces, seed):
    """n_faces random faces with three distinct indices over a few more vertices than a closed surface would have."""
    rng = np.random.default_rng(seed)
    n_vertices = 0 if n_faces == 0 else n_faces // 2 + 3
    vertices = rng.uniform(-40, 40, (n_vertices, 3)).astype(F)
    return vertices, (_distinct_triples(rng, n_vertices, n_faces) if n_faces else np.zeros((0, 3), np.int32))


def degenerate(seed=7):
    """200 vertices / 800 faces: 600 random triples of distinct indices, and shuffled among them faces that must go: a repeated index,
    two indices with bit-equal positions, three collinear vertices, indices >= n_vertices and < 0, and a NaN vertex used by 60 faces.
    20 vertices lie at x = 0 exactly (w' = 0 under the projective transform)."""
    rng = np.random.default_rng(seed)
    n = 200
    v = rng.uniform(-40, 40, (n, 3)).astype(F)
    v[20:40, 0] = 0.0                      # w' = 0 under a last row (1, 0, 0, 0)
    v[180:190] = v[0:10]                   # bit-equal copies of vertices 0..9
    t = np.arange(10, dtype=F)
    v[170:180] = np.stack([F(1.0) + t, F(2.0) + F(2.0) * t, F(-3.0) + F(4.0) * t], axis=1)  # on one line, exactly
    nan_vertex = 199
    v[nan_vertex, 0] = np.nan
    faces = [_distinct_triples(rng, 170, 600)]
    a = rng.integers(0, 170, 40)
    b = (a + 1 + rng.integers(0, 168, 40)) % 170
    faces.append(np.stack([a, b, np.where(rng.integers(0, 2, 40) == 1, a, b)], axis=1))                  # a repeated index
    k = rng.integers(0, 10, 40)
    faces.append(np.stack([k, 180 + k, 40 + rng.integers(0, 100, 40)], axis=1)[:, rng.permutation(3)])   # two bit-equal positions
    faces.append(np.stack([170 + rng.choice(10, 3, replace=False) for _ in range(20)]))                  # collinear
    faces.append(np.stack([rng.integers(0, 170, 20), n + rng.integers(0, 1000, 20), rng.integers(0, 170, 20)], axis=1))  # >= n_vertices
    faces.append(np.stack([rng.integers(0, 170, 20), rng.integers(0, 170, 20), -1 - rng.integers(0, 50, 20)], axis=1))   # < 0
    faces.append(np.stack([np.full(60, nan_vertex), rng.integers(0, 80, 60), 80 + rng.integers(0, 80, 60)], axis=1))     # the NaN vertex
    faces = np.concatenate(faces).astype(np.int32)
    assert len(faces) == 800
    return v, faces[rng.permutation(len(faces))]


def smoothing(seed=11):
    """A 96-face fan around vertex 0 over a rim that is not flat (valence > 64; its normal sum depends on the order of the additions),
    a face and its reversed copy on vertices 98, 99, 100 (their unit normals cancel exactly), a third face on 98 and 99 (so only 100
    keeps a zero sum and with it its face normals), vertex 101 of valence 1 and the unused vertex 102."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0.0, 1.9 * np.pi, 97)
    rim = np.stack([10 * np.cos(ang), rng.uniform(-3, 3, 97), 10 * np.sin(ang)], axis=1)
    v = np.concatenate([[[0.0, 4.0, 0.0]], rim, rng.uniform(20, 30, (5, 3))]).astype(F)
    fan = np.stack([np.zeros(96, np.int32), np.arange(1, 97), np.arange(2, 98)], axis=1)
    extra = np.array([[98, 99, 100], [98, 100, 99], [98, 99, 101]])
    return v, np.concatenate([fan, extra]).astype(np.int32)


SMOOTHING_SKIPPED_VERTEX, SMOOTHING_FAN_VERTEX, SMOOTHING_UNUSED_VERTEX = 100, 0, 102

MESHES = {
    "empty": (np.zeros((0, 3), F), np.zeros((0, 3), np.int32)),
    "faces0": (np.random.default_rng(1).uniform(-1, 1, (5, 3)).astype(F), np.zeros((0, 3), np.int32)),
    "faces1": sized(1, 2),
    "faces63": sized(63, 3),
    "faces64": sized(64, 4),
    "faces65": sized(65, 5),
    "faces257": sized(257, 6),
    "degenerate": degenerate(),
    "smoothing": smoothing(),
}

TRANSFORMS = {
    "identity": np.eye(4, dtype=F),
    "scale_translate": np.array([[0.01, 0, 0, 0.1], [0, 0.02, 0, -0.5], [0, 0, 0.01, 0.3], [0, 0, 0, 1]], F),  # the loader test's
    "mirror": np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F),
    "flatten": np.array([[1, 0, 0, 0], [0, 0, 0, 2], [0, 0, 1, 0], [0, 0, 0, 1]], F),
    "projective": np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]], F),
    "tiny": np.diag(np.array([1e-20, 1e-20, 1e-20, 1], F)),
    "huge": np.diag(np.array([1e20, 1e20, 1e20, 1], F)),
}

CASES = [(m, t, s) for m in MESHES for t in TRANSFORMS for s in (0, 1)]


def case_key(mesh, transform, smooth):
    return "%s__%s__%d" % (mesh, transform, smooth)


def obj_text(vertices, faces):
    lines = []
    for x, y, z in np.asarray(vertices, F).tolist():
        lines.append("v %s %.9g %.9g" % ("-" if x != x else "%.9g" % x, y, z))
    for a, b, c in np.asarray(faces).tolist():
        lines.append("f %d %d %d" % (a + 1, b + 1, c + 1))
    return ("\n".join(lines) + "\n").encode()


def load_mesh(lib, prefix, vertices, faces, matrix, smooth):
    """io::loadMesh of the host library (prefix 'pth_') or of the compiled reference ('ref_') on the mesh's OBJ text: (count, positions
    (count, 9), normals (count, 9))."""
    fn = getattr(lib, prefix + "load_mesh")
    fn.restype = C.c_uint64
    text = obj_text(vertices, faces)
    cap = max(len(faces), 1)
    pos, nrm = np.zeros((cap, 9), F), np.zeros((cap, 9), F)
    m = np.ascontiguousarray(matrix, F)
    n = fn(C.c_char_p(text), C.c_uint64(len(text)), C.c_void_p(m.ctypes.data), C.c_int(smooth), C.c_uint64(cap), C.c_void_p(pos.ctypes.data), C.c_void_p(nrm.ctypes.data))
    assert n <= cap
    return int(n), pos[:n].copy(), nrm[:n].copy()


def share_conditions(n_kept, n_faces=800):
    """The degenerate family must both drop and keep a real share: between 10 % and 50 % of the faces dropped, at least 400 kept."""
    dropped = n_faces - n_kept
    assert 0.10 * n_faces <= dropped <= 0.50 * n_faces, (n_kept, n_faces)
    assert n_kept >= 400, n_kept


def smoothing_conditions(vertices, faces, nrm_flat, nrm_smooth):
    """On an untransformed answer for the smoothing family: at least one vertex was skipped (kept its face normals although it has
    faces), one was smoothed, and one has valence >= 65.  All its faces survive, so corner (j, s) belongs to vertex faces[j, s]."""
    assert len(nrm_flat) == len(faces) == len(nrm_smooth)
    valence = np.bincount(faces.ravel(), minlength=len(vertices))
    same = (nrm_flat.reshape(-1, 3, 3).view(np.uint32) == nrm_smooth.reshape(-1, 3, 3).view(np.uint32)).all(axis=2)  # (face, slot)
    skipped = [v for v in range(len(vertices)) if valence[v] > 0 and same[faces == v].all()]
    smoothed = [v for v in range(len(vertices)) if valence[v] > 1 and not same[faces == v].any()]
    assert SMOOTHING_SKIPPED_VERTEX in skipped, skipped
    assert SMOOTHING_FAN_VERTEX in smoothed and valence[SMOOTHING_FAN_VERTEX] >= 65, (smoothed, valence[:2])
    assert valence[SMOOTHING_UNUSED_VERTEX] == 0 and (valence == 1).any()


def guarded(rows, width=9):
    """A (rows, width) float32 array between two bands of GUARD_ROWS rows of 0xA5 bytes: (whole, view of the rows)."""
    whole = np.full((rows + 2 * GUARD_ROWS) * width * 4, 0xA5, np.uint8).view(F).reshape(-1, width)
    return whole, whole[GUARD_ROWS:GUARD_ROWS + rows]


def assert_guards(whole, rows, written, what):
    """Nothing outside the first `written` rows was touched."""
    raw = whole.view(np.uint8).reshape(len(whole), -1)
    assert (raw[:GUARD_ROWS] == 0xA5).all() and (raw[GUARD_ROWS + written:] == 0xA5).all(), what
