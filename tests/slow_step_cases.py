"""Edge vectors for the triangle test as straight-line code (pt_device.h: tri_intersect), in the layouts of oracle.Checker.tri_intersect.

The reference leaves Triangle::getIntersection through three early returns; the device evaluates all of it and selects -1 on the same
predicates.  These vectors sit ON those predicates and beyond what the early returns used to shield: a determinant of exactly 0 (the
division then yields inf, the products NaN), determinants at +-1e-6 and one ulp either side with both cull values, barycentrics that are
exactly 0, exactly 1 and their neighbours (rays through a vertex, through a shared edge, u + v = 1), triangles without area, hits behind the
origin, directions with zero components, and inputs that make u or v NaN (which fails none of the reference's tests).

The constructed part uses a = (0, 0, 0), ab = (s, 0, 0), ac = (0, 1, 0), o = (x, y, 1), d = (0, 0, -e), for which every product is exact:
pvec = (e, 0, 0), det = s e, u = x e / det, qvec = (0, s, -s y), v = s y e / det, t = s / det.  With s = 1: det = e, u = x, v = y, t = 1 / e.
tests/test_slow_step_cases_cpu.py holds the C oracle equal to the compiled reference on these arrays, tests/test_gpu_slow_step.py the device
equal to the oracle."""
import numpy as np

from tests.unit_cases import ulp_step, unit

F = np.float32
EPS = np.float32(1e-6)  # the literal of object.cpp:151 as a float


def _pack(a, b, c, o, d):
    n = max(len(np.atleast_2d(x)) for x in (a, b, c, o, d))
    cols = [np.broadcast_to(np.atleast_2d(np.asarray(x, dtype=F)), (n, 3)) for x in (a, b, c, o, d)]
    return np.concatenate(cols[:3], axis=1).astype(F), np.concatenate(cols[3:], axis=1).astype(F)


def determinant_vectors():
    """det = e exactly: 0, -0, denormals, +-1e-6 and up to two ulp either side, +-1; each with the ray through the inside (0.25, 0.25),
    through the vertex a and through the edge u + v = 1."""
    e = [F(0.0), F(-0.0), F(1.4e-45), F(-1.4e-45), F(1e-38), F(-1e-38), F(1.0), F(-1.0), F(3e38), F(-3e38)]
    for k in (-2, -1, 0, 1, 2):
        e.append(ulp_step(np.array([EPS]), k)[0])
        e.append(-ulp_step(np.array([EPS]), k)[0])
    e = np.array(e, dtype=F)
    xy = np.array([[0.25, 0.25], [0.0, 0.0], [0.5, 0.5]], dtype=F)
    ee, pp = np.meshgrid(np.arange(len(e)), np.arange(len(xy)), indexing="ij")
    ee, pp = ee.ravel(), pp.ravel()
    n = len(ee)
    o = np.stack([xy[pp, 0], xy[pp, 1], np.ones(n, F)], axis=1)
    d = np.stack([np.zeros(n, F), np.zeros(n, F), -e[ee]], axis=1)
    return _pack([0, 0, 0], [1, 0, 0], [0, 1, 0], o, d)


def barycentric_vectors():
    """det = 1 and det = -1 (the back face); (u, v) = (x, y) over 0, -0, the denormals and ulps around 0, 0.25, 0.5, 0.75 and the ulps around 1:
    vertices (0, 0), (1, 0), (0, 1), the three edges, and u + v landing on, below and above 1."""
    one = np.array([F(1.0)])
    grid = np.array([0.0, -0.0, 1.4e-45, -1.4e-45, 1e-38, -1e-38, 0.25, 0.5, 0.75,
                     ulp_step(one, -2)[0], ulp_step(one, -1)[0], 1.0, ulp_step(one, 1)[0], ulp_step(one, 2)[0],
                     ulp_step(np.array([F(0.5)]), -1)[0], ulp_step(np.array([F(0.5)]), 1)[0], ulp_step(np.array([F(0.25)]), 1)[0],
                     ulp_step(np.array([F(0.75)]), -1)[0], ulp_step(np.array([F(0.75)]), 1)[0]], dtype=F)
    x, y = [g.ravel() for g in np.meshgrid(grid, grid, indexing="ij")]
    n = len(x)
    tri, rays = [], []
    for side in (F(-1.0), F(1.0)):  # d = (0, 0, side): det = -side
        o = np.stack([x, y, np.full(n, -side, F)], axis=1)
        t_, r_ = _pack([0, 0, 0], [1, 0, 0], [0, 1, 0], o, [0, 0, side])
        tri.append(t_)
        rays.append(r_)
    return np.concatenate(tri), np.concatenate(rays)


def shared_edge_vectors(seed=11, n=600):
    """Two triangles (a, b, c) and (b, a, c') that share the edge a-b, all coordinates small dyadic rationals (every difference exact), and
    rays from both sides aimed at float points of the shared edge and at its two vertices: each ray is tested against BOTH triangles."""
    rng = np.random.default_rng(seed)
    q = 1.0 / 64.0
    a = rng.integers(-64, 64, (n, 3)) * q
    b = a + rng.integers(-32, 33, (n, 3)) * q
    c = a + rng.integers(-32, 33, (n, 3)) * q
    c2 = a + b - c  # the mirror image of c through the edge's midpoint
    w = rng.integers(0, 9, n)[:, None] / 8.0  # 0 and 1: the vertices
    target = a + (b - a) * w
    o = target + rng.integers(-64, 65, (n, 3)) * q * 2.0
    with np.errstate(invalid="ignore"):
        d = unit(target - o)
    d = np.where(np.isfinite(d), d, 0.0)
    t1, r1 = _pack(a, b, c, o, d)
    t2, r2 = _pack(b, a, c2, o, d)
    return np.concatenate([t1, t2]), np.concatenate([r1, r2])


def degenerate_vectors(seed=12, n=300):
    """Triangles without area (b = a; c = a; a = b = c; c on the line a-b, beyond b and between), hit head-on and in their plane."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, (n, 3)) / 8.0
    ab = rng.integers(-8, 9, (n, 3)) / 8.0
    kind = np.arange(n) % 5
    b = np.where((kind == 0)[:, None] | (kind == 2)[:, None], a, a + ab)
    c = np.select([(kind == 1)[:, None], (kind == 2)[:, None], (kind == 3)[:, None], (kind == 4)[:, None]], [a, a, a + 2.0 * ab, a + 0.5 * ab], a + ab[:, ::-1])
    o = a + rng.integers(-16, 17, (n, 3)) / 8.0
    target = a + ab * (rng.integers(0, 5, n)[:, None] / 4.0)
    with np.errstate(invalid="ignore"):
        d = unit(target - o)
    d = np.where(np.isfinite(d), d, 0.0)
    return _pack(a, b, c, o, d)


def behind_and_axis_vectors(seed=13, n=600):
    """General triangles (dyadic coordinates); rays along +-x, +-y, +-z and with two zero components replaced by +-0, from in front of the triangle,
    from behind it (t < 0), from a point ON it (t = 0) and all-zero directions."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-16, 17, (n, 3)) / 16.0
    b = a + rng.integers(-16, 17, (n, 3)) / 16.0
    c = a + rng.integers(-16, 17, (n, 3)) / 16.0
    u, v = rng.integers(0, 5, n) / 8.0, rng.integers(0, 5, n) / 8.0  # inside or on the edge u + v = 1 ... never beyond
    target = a + (b - a) * u[:, None] + (c - a) * v[:, None]
    axis = rng.integers(0, 3, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    d = np.zeros((n, 3))
    d[np.arange(n), axis] = sign
    d = np.where(d == 0, np.where(rng.random((n, 3)) < 0.5, -0.0, 0.0), d)
    back = rng.choice([-2.0, -0.5, 0.0, 0.5, 2.0], n)  # the origin at target - back * d: back < 0 puts the hit behind it
    o = target - d * back[:, None]
    d[::37] = 0.0
    return _pack(a, b, c, o, d)


def nan_vectors():
    """Inputs for which the reference computes u or v as NaN and goes on (NaN < 0 and NaN > 1 are false): an infinite determinant (inv_det = 0 times
    an infinite dot product), NaN and infinite origins with a finite determinant (u NaN; with the NaN confined to one component, v NaN and u finite),
    products that overflow to inf - inf, and NaN in the triangle and in the direction (det NaN: it fails neither epsilon test)."""
    nan, inf, big = F(np.nan), F(np.inf), F(3e38)
    tri, rays, a0, b0, c0 = [], [], [0, 0, 0], [1, 0, 0], [0, 1, 0]

    def add(a, b, c, o, d):
        t_, r_ = _pack(a, b, c, o, d)
        tri.append(t_)
        rays.append(r_)

    for x in (nan, inf, -inf, big, -big):
        for k in range(3):
            o = np.array([0.25, 0.25, 1.0], dtype=F)
            o[k] = x
            add(a0, b0, c0, o, [0, 0, -1])   # det = 1: the division is ordinary, u or v is not
            add(a0, b0, c0, o, [0, 0, 1])    # det = -1
            add(a0, b0, c0, o, [0.5, 0.25, -1])
    for s in (big, -big, F(1e30), F(1e20)):
        add(a0, [s, 0, 0], [0, s, 0], [0.25, 0.25, 1.0], [0, 0, -s])   # pvec overflows: det = +-inf, inv_det = +-0
        add(a0, [s, 0, 0], [0, 1, 0], [s, s, s], [0, 0, -1])            # qvec = inf - inf
        add([s, s, s], [-s, s, 0], [0, -s, s], [0, 0, 0], [1, 1, 1])    # differences overflow
        add(a0, b0, c0, [0.25, 0.25, 1.0], [s, s, -s])
    for k in range(3):
        v = np.zeros(3, F)
        v[k] = nan
        add(v, b0, c0, [0.25, 0.25, 1.0], [0, 0, -1])
        add(a0, np.array(b0, F) + v, c0, [0.25, 0.25, 1.0], [0, 0, -1])
        add(a0, b0, np.array(c0, F) + v, [0.25, 0.25, 1.0], [0, 0, -1])
        add(a0, b0, c0, [0.25, 0.25, 1.0], np.array([0, 0, -1], F) + v)
    return np.concatenate(tri), np.concatenate(rays)


FAMILIES = (("determinant", determinant_vectors), ("barycentric", barycentric_vectors), ("shared_edge", shared_edge_vectors),
            ("degenerate", degenerate_vectors), ("behind_axis", behind_and_axis_vectors), ("nan", nan_vectors))


def edge_vectors():
    """{family: (tri (n, 9), cull (n,) uint8, rays (n, 6))}: every vector of every family with both cull values."""
    out = {}
    for name, make in FAMILIES:
        tri, rays = make()
        n = len(tri)
        out[name] = (np.ascontiguousarray(np.concatenate([tri, tri])), np.concatenate([np.zeros(n, np.uint8), np.ones(n, np.uint8)]),
                     np.ascontiguousarray(np.concatenate([rays, rays])))
    return out


def stages(tri, rays):
    """(det, u, v) of Triangle::getIntersection evaluated in float32 in the reference's order, WITHOUT its early returns: what a vector exercises
    (used to check that a family contains what its name says, never as an expected result)."""
    tri, rays = np.asarray(tri, F), np.asarray(rays, F)
    with np.errstate(all="ignore"):
        a, ab, ac, o, d = tri[:, 0:3], tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3], rays[:, 0:3], rays[:, 3:6]

    def cross(p, q):
        return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], axis=1).astype(F)

    def dot(p, q):
        return ((F(0.0) + p[:, 0] * q[:, 0]) + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]

    with np.errstate(all="ignore"):
        pvec = cross(d, ac)
        det = dot(ab, pvec)
        inv = F(1.0) / det
        tvec = (o - a).astype(F)
        u = dot(tvec, pvec) * inv
        v = dot(d, cross(tvec, ab)) * inv
    return det, u, v
