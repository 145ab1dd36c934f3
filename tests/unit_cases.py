"""Edge-case inputs for the unit functions of the hot path (slab test, triangle, sphere, BSDFs, camera, engine, device libm).

Every generator is deterministic from its seed and returns float32 / integer arrays in the layouts of oracle.Checker, so the same
arrays go to the compiled reference, the C oracle (tests/test_unit_cases_cpu.py) and the device probe (tests/test_gpu_units.py).
Each family mixes the constructions that make a restated function diverge (exact zeros, one-ulp neighbours of a branch point,
denormals, huge and tiny scales) with plain random cases; constructions are formed in float64 and rounded once.
"""
import numpy as np

F = np.float32
DENORM_MIN = np.float32(1.401298464324817e-45)
U64_MAX = 0xFFFFFFFFFFFFFFFF
FLT_MAX = np.finfo(np.float32).max


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def ulp_step(a, k):
    """float32 array `a` moved by k representable values (k an integer or integer array; crosses zero correctly)."""
    a = np.ascontiguousarray(a, dtype=F)
    i = a.view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7FFFFFFF), i)  # ordered integers: -0 and +0 both map to 0
    i = i + k
    out = np.where(i < 0, (-i) | 0x80000000, i).astype(np.uint32)
    return out.view(F).reshape(a.shape)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):  # (whole-array constructions leave zero rows in the parts that do not use them)
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_dirs(rng, n):
    return unit(rng.normal(size=(n, 3)))


def perpendicular(rng, d):
    """A random float64 unit vector perpendicular to each row of d."""
    r = rng.normal(size=d.shape)
    return unit(np.cross(d, r))


def _parts(n, k):
    """k slice objects that split range(n) into nearly equal consecutive parts."""
    edges = [n * i // k for i in range(k + 1)]
    return [slice(edges[i], edges[i + 1]) for i in range(k)]


def rng_states(rng, n):
    """Engine states: random, with 0 (the engine's fixed point) and 2^64 - 1 mixed in."""
    st = rng.integers(0, U64_MAX, size=n, dtype=np.uint64, endpoint=True)
    st[::17] = 0
    st[5::17] = U64_MAX
    return st


# ---- slab_test / slab_walk ---------------------------------------------------------------------------------------------------

def slab_family(seed, n=60000):
    """boxes (n, 6), rays (n, 6).  Parts: random | direction components +-0 | denormal direction components (inverse = inf) | origin on
    a face plane | flat boxes | origin inside / box behind | along edges and through corners | coordinates at 1e-38, 1e-30, 1e30."""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-1, 1, (n, 3))
    hi = lo + rng.uniform(0.05, 1, (n, 3))
    o = rng.uniform(-3, 3, (n, 3))
    target = lo + (hi - lo) * rng.uniform(-0.4, 1.4, (n, 3))  # inside the box about a third of the time
    d = unit(target - o)
    parts = _parts(n, 8)
    axis = rng.integers(0, 3, n)
    rows = np.arange(n)

    # (1) direction components exactly +-0: the origin sits over the box in those axes half of the time
    s = parts[1]
    zero = rng.random((n, 3)) < 0.45
    zero[rows, axis] = False  # (keep one component)
    inside = lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3))
    oz = np.where(zero & (rng.random((n, 3)) < 0.7), inside, o)
    dz = np.where(zero, 0.0, target - oz)
    dz = unit(np.where(np.abs(dz).sum(axis=1, keepdims=True) > 0, dz, 1.0))
    dz = np.where(zero, np.where(rng.random((n, 3)) < 0.5, -0.0, 0.0), dz)
    o[s], d[s] = oz[s], dz[s]

    # (2) denormal direction components: 1 / d overflows to +-inf, and (face - origin) = 0 makes 0 * inf = NaN
    s = parts[2]
    tiny = np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0) * rng.choice([1.4e-45, 1e-42, 2.9e-39], (n, 3))
    dd = np.where(zero, tiny, dz)
    on_face = zero & (rng.random((n, 3)) < 0.08)
    od = np.where(on_face, np.where(rng.random((n, 3)) < 0.5, lo, hi), oz)
    o[s], d[s] = od[s], dd[s]

    # (3) origin exactly on a face plane (one axis), looking in or out or along the face
    s = parts[3]
    of = o.copy()
    of[rows, axis] = np.where((rng.random(n) < 0.5)[:, None], lo, hi)[rows, axis]
    df = unit(target - of)
    along = rng.random(n) < 0.3
    df[along, axis[along]] = 0.0
    df = unit(df)
    o[s], d[s] = of[s], df[s]

    # (4) boxes flat on one, two or three axes, rays aimed at (or just past) them
    s = parts[4]
    flat = rng.random((n, 3)) < 0.5
    flat[rows, axis] = True
    hf = np.where(flat, lo, hi)
    aim = lo + (hf - lo) * rng.uniform(-0.2, 1.2, (n, 3))
    snap = rng.random(n) < 0.5  # axis-parallel rays straight at the flat box
    ofl = np.where(snap[:, None], aim, o)
    ofl[rows, axis] = o[rows, axis]
    dfl = unit(aim - ofl)
    hi[s], o[s], d[s] = hf[s], ofl[s], dfl[s]

    # (5) origin inside the box; box behind the origin
    s = parts[5]
    behind = rng.random(n) < 0.5
    oi = np.where(behind[:, None], o, inside)
    di = np.where(behind[:, None], -unit(target - o), random_dirs(rng, n))
    o[s], d[s] = oi[s], di[s]

    # (6) rays through corners and along edges (float32 corner coordinates, so that the differences are exact where they can be)
    s = parts[6]
    lo32, hi32 = lo.astype(F).astype(np.float64), hi.astype(F).astype(np.float64)
    corner = np.where(rng.random((n, 3)) < 0.5, lo32, hi32)
    edge = rng.random(n) < 0.5
    oc = o.copy()
    dc = unit(corner - oc)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    oe = corner.copy()
    oe[rows, axis] = corner[rows, axis] - sign * rng.uniform(0.5, 2.0, n)
    de = np.zeros((n, 3))
    de[rows, axis] = sign * np.where(rng.random(n) < 0.8, 1.0, -1.0)
    oc, dc = np.where(edge[:, None], oe, oc), np.where(edge[:, None], de, dc)
    lo[s], hi[s], o[s], d[s] = lo32[s], hi32[s], oc[s], dc[s]

    # (7) the whole configuration at 1e-38 (denormal differences), 1e-30 and 1e30
    s = parts[7]
    scale = rng.choice([1e-38, 1e-30, 1e30], n)[:, None]
    lo[s], hi[s], o[s] = (lo * scale)[s], (hi * scale)[s], (o * scale)[s]

    boxes = np.concatenate([lo, hi], axis=1).astype(F)
    rays = np.concatenate([o, d], axis=1).astype(F)
    return boxes, rays


def slab_nan_mask(boxes, rays):
    """True where one of the six slab products is NaN (the cases slab_walk is documented to treat differently), computed as the slab test
    computes them, in float32."""
    boxes, rays = np.asarray(boxes, F), np.asarray(rays, F)
    lo, hi, o, d = boxes[:, :3], boxes[:, 3:], rays[:, :3], rays[:, 3:]
    with np.errstate(all="ignore"):
        inv = np.where(np.abs(d) > 0, F(1.0) / np.where(d == 0, F(1.0), d), FLT_MAX).astype(F)
        t = np.concatenate([(lo - o) * inv, (hi - o) * inv], axis=1)
    return np.isnan(t).any(axis=1)


# ---- tri_intersect / tri_normal ----------------------------------------------------------------------------------------------

def triangle_family(seed, n=60000):
    """tri (n, 9), cull (n,), rays (n, 6), nrm (n, 9), pos (n, 3).  Parts: random | aimed at vertices and edge points | rays in the
    triangle's plane (determinant 0 and +-denormal) | zero-area and collinear | both sides, both cull values | origin on the triangle and
    just behind it | 1e-20 and 1e20 scales (which overflow or flush the products) beside 1e-3 and 1e3."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, 3))
    b = a + rng.uniform(-1, 1, (n, 3))
    c = a + rng.uniform(-1, 1, (n, 3))
    cull = (rng.random(n) < 0.5).astype(np.uint8)
    u = rng.uniform(-0.25, 0.9, n)
    v = rng.uniform(-0.25, 0.9, n)
    o = a + rng.uniform(-2, 2, (n, 3))
    parts = _parts(n, 7)

    def f32(x):
        return x.astype(F).astype(np.float64)

    # (1) aimed exactly at the vertices and at points of the edges: barycentrics 0, 1 and their neighbours
    s = parts[1]
    which = rng.integers(0, 6, n)
    e = rng.uniform(0, 1, n)
    u1 = np.select([which == 0, which == 1, which == 2, which == 3, which == 4], [0 * e, 1 + 0 * e, 0 * e, e, 0 * e], 1 - e)
    v1 = np.select([which == 0, which == 1, which == 2, which == 3, which == 4], [0 * e, 0 * e, 1 + 0 * e, 0 * e, e], e)
    u[s], v[s] = u1[s], v1[s]
    a[s], b[s], c[s], o[s] = f32(a)[s], f32(b)[s], f32(c)[s], f32(o)[s]
    target = a + (b - a) * u[:, None] + (c - a) * v[:, None]
    d = unit(target - o)

    # (2) rays in the triangle's plane.  Axis-aligned planes make the determinant exactly 0; a denormal normal component makes it +-denormal.
    s = parts[2]
    k = rng.integers(0, 3, n)
    rows = np.arange(n)
    ap, bp, cp, op = f32(a), f32(b), f32(c), f32(o)
    plane = rng.uniform(-1, 1, n).astype(F).astype(np.float64)
    for arr in (ap, bp, cp, op):
        arr[rows, k] = plane
    dp = unit(target - op)
    dp[rows, k] = 0.0
    dp = unit(np.where(np.abs(dp).sum(axis=1, keepdims=True) > 0, dp, 1.0))
    dp[rows, k] = rng.choice([0.0, -0.0, 1.4e-45, -1.4e-45, 1e-39, -1e-39, 1e-7, -1e-7], n)
    general = rng.random(n) < 0.3  # a general plane: the determinant is a rounding residue
    og = a + (b - a) * rng.uniform(-1, 2, (n, 1)) + (c - a) * rng.uniform(-1, 2, (n, 1))
    ap, bp, cp = (np.where(general[:, None], x, y) for x, y in ((a, ap), (b, bp), (c, cp)))
    op, dp = np.where(general[:, None], og, op), np.where(general[:, None], unit(target - og + 1e-300), dp)
    a[s], b[s], c[s], o[s], d[s] = ap[s], bp[s], cp[s], op[s], dp[s]

    # (3) zero-area and collinear triangles
    s = parts[3]
    kind = rng.integers(0, 4, n)
    bz = np.select([kind[:, None] == 0, kind[:, None] == 3], [a, a], b)
    cz = np.select([kind[:, None] == 1, kind[:, None] == 2, kind[:, None] == 3], [a, f32(a) + (f32(b) - f32(a)) * 2.0, a], c)
    az = np.where(kind[:, None] == 2, f32(a), a)
    bz = np.where(kind[:, None] == 2, f32(b), bz)
    a[s], b[s], c[s] = az[s], bz[s], cz[s]

    # (4) both cull values from both sides: the same ray and its mirror image through the target
    s = parts[4]
    flip = rng.random(n) < 0.5
    om = np.where(flip[:, None], 2 * target - o, o)
    o[s], d[s] = om[s], unit(target - om)[s]

    # (5) origin on the triangle (t = 0) and just behind it along the ray
    s = parts[5]
    ui, vi = rng.uniform(0.05, 0.45, n), rng.uniform(0.05, 0.45, n)
    on = f32(a) + (f32(b) - f32(a)) * ui[:, None] + (f32(c) - f32(a)) * vi[:, None]
    dn = random_dirs(rng, n)
    back = rng.choice([0.0, 0.0, 1e-7, 1e-6, -1e-7, 1e-4], n)[:, None]
    a[s], b[s], c[s], o[s], d[s] = f32(a)[s], f32(b)[s], f32(c)[s], (on + dn * back)[s], dn[s]

    # (6) the whole configuration at 1e-20 and 1e20, and at 1e-3 and 1e3 where the results stay finite
    s = parts[6]
    scale = rng.choice([1e-20, 1e20, 1e-3, 1e3], n)[:, None]
    a[s], b[s], c[s], o[s] = (a * scale)[s], (b * scale)[s], (c * scale)[s], (o * scale)[s]

    tri = np.concatenate([a, b, c], axis=1).astype(F)
    rays = np.concatenate([o, d], axis=1).astype(F)
    nrm = np.concatenate([random_dirs(rng, n) for _ in range(3)], axis=1).astype(F)
    # surface points for tri_normal: where the rays were aimed (vertices, edges, in-plane points, degenerate triangles included)
    t32 = tri.astype(np.float64)
    pos = (t32[:, 0:3] + (t32[:, 3:6] - t32[:, 0:3]) * u[:, None] + (t32[:, 6:9] - t32[:, 0:3]) * v[:, None]).astype(F)
    return tri, cull, rays, nrm, pos


# ---- sphere_intersect --------------------------------------------------------------------------------------------------------

def sphere_family(seed, n=40000):
    """sph (n, 4), rays (n, 6).  Parts: random | tangent rays, the radius then moved by 0, +-1, +-2 ulp | tangent rays, an origin
    coordinate moved | origin at the centre, on the surface, inside, beyond | radii 1e-6 and 1e6."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1, 1, (n, 3))
    radius = rng.uniform(0.1, 1.0, n)
    parts = _parts(n, 5)
    s = parts[4]
    radius[s] = rng.choice([1e-6, 1e6], n)[s]
    centre32 = centre.astype(F).astype(np.float64)
    radius32 = radius.astype(F).astype(np.float64)
    dist = radius32 * rng.uniform(1.2, 4.0, n)
    away = random_dirs(rng, n)
    o = centre32 + away * dist[:, None]
    # aim at a point within 1.6 radii of the centre, in the plane through the centre perpendicular to the line of sight
    side = perpendicular(rng, away)
    off = rng.uniform(0, 1.6, n)
    d = unit(centre32 + side * (off * radius32)[:, None] - o)

    # tangent rays: the angle between the ray and the line to the centre has sine radius / distance
    sin_t = radius32 / dist
    tangent = -away * np.sqrt(1 - sin_t ** 2)[:, None] + side * sin_t[:, None]
    o32 = o.astype(F)
    d[parts[1]], d[parts[2]] = tangent[parts[1]], tangent[parts[2]]
    k = rng.integers(-2, 3, n)
    r_out = radius32.astype(F)
    r_out[parts[1]] = ulp_step(r_out, k)[parts[1]]
    axis = rng.integers(0, 3, n)
    rows = np.arange(n)
    moved = o32.copy()
    moved[rows, axis] = ulp_step(o32[rows, axis], k)
    o32[parts[2]] = moved[parts[2]]
    d[parts[4]] = np.where((rng.random(n) < 0.5)[:, None], tangent, d)[parts[4]]

    # origin at the centre, on the surface, inside, beyond (the sphere behind the ray)
    s = parts[3]
    where = rng.integers(0, 4, n)
    frac = np.select([where == 0, where == 1, where == 2], [0 * dist, 1 + 0 * dist, rng.uniform(0, 1, n)], dist / radius32)
    os_ = (centre32 + away * (frac * radius32)[:, None]).astype(F)
    ds = np.where((where == 3)[:, None], np.where((rng.random(n) < 0.7)[:, None], away, d), random_dirs(rng, n))
    o32[s], d[s] = os_[s], ds[s]

    sph = np.concatenate([centre32, r_out[:, None].astype(np.float64)], axis=1).astype(F)
    rays = np.concatenate([o32.astype(np.float64), d], axis=1).astype(F)
    return sph, rays


# ---- bsdf_propagate ----------------------------------------------------------------------------------------------------------

IORS = np.array([1.0, np.nextafter(F(1.0), F(2.0)), 1.05, 1.5, 2.5], dtype=F)
EPSILONS = [1e-2, 1e-3, 1e-4]
BSDF_KINDS = [("lambert", 0, 0), ("glass", 1, 0), ("mirror", 2, 0), ("mirror1", 2, 1)]
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)


def axis_normals(rng, n):
    """+-x, +-y, +-z and their neighbours: the unit component one ulp below 1, the others 0, -0, +-denormal or +-1e-30 (every branch of
    local_to_global, on both sides of its `> 0` tests)."""
    ax = AXES[rng.integers(0, 6, n)]
    small = rng.choice([0.0, -0.0, 1.4e-45, -1.4e-45, 1e-30, -1e-30], (n, 3))
    nrm = np.where(ax != 0, ax, small).astype(F)
    below = rng.random(n) < 0.3
    nrm = np.where(below[:, None] & (ax != 0), ulp_step(nrm, -np.sign(ax).astype(np.int64)), nrm)
    return nrm


def bsdf_propagate_family(seed, n=24000):
    """rays (n, 6), pos (n, 3), nrm (n, 3), ior (n,), states (n,).  Parts: random | d perpendicular to n, exactly and with dot(n, d) of
    +-1 ulp | d = -n and d = n | axis normals and their neighbours | glass at the critical angle +-{0, 1, 2} ulp, from inside and outside."""
    rng = np.random.default_rng(seed)
    nrm = random_dirs(rng, n)
    d = random_dirs(rng, n)
    ior = IORS[rng.integers(0, len(IORS), n)]
    parts = _parts(n, 6)

    # (1) perpendicular: axis pairs give dot = 0 exactly; a denormal component along the normal gives dot = +-denormal
    s = parts[1]
    i = rng.integers(0, 6, n)
    j = (i // 2 * 2 + 2 + 2 * rng.integers(0, 2, n) + rng.integers(0, 2, n)) % 6
    n_ax, d_ax = AXES[i], AXES[j].copy()
    d_ax = d_ax + n_ax * rng.choice([0.0, 0.0, 1.4e-45, -1.4e-45, 1e-38, -1e-38], n)[:, None]
    general = rng.random(n) < 0.4  # a general normal: dot(n, d) is a rounding residue of either sign
    nrm[s] = np.where(general[:, None], nrm, n_ax)[s]
    d[s] = np.where(general[:, None], perpendicular(rng, nrm), d_ax)[s]

    # (2) head-on and from behind
    s = parts[2]
    n32 = nrm.astype(F).astype(np.float64)
    nrm[s] = n32[s]
    d[s] = np.where((rng.random(n) < 0.7)[:, None], -n32, n32)[s]

    # (3) axis normals and their one-ulp neighbours, random directions (some of them along another axis)
    s = parts[3]
    nrm[s] = axis_normals(rng, n).astype(np.float64)[s]
    d[s] = np.where((rng.random(n) < 0.25)[:, None], AXES[rng.integers(0, 6, n)], d)[s]

    # (4, 5) the critical angle: sin(theta_i) = 1 / ior seen from inside (dot(d, n) > 0); from outside the refracted sine reaches 1 only
    # at grazing incidence for ior = 1.  One component of d is then moved by 0, +-1, +-2 ulp.
    s = slice(parts[4].start, parts[5].stop)
    nc = np.where((rng.random(n) < 0.5)[:, None], AXES[rng.integers(0, 6, n)], nrm.astype(F).astype(np.float64))
    sin_i = np.minimum(1.0 / ior.astype(np.float64), 1.0)
    cos_i = np.sqrt(np.maximum(1.0 - sin_i ** 2, 0.0))
    side = np.where(rng.random(n) < 0.6, 1.0, -1.0)  # +1: inside the glass
    dc = (nc * (side * cos_i)[:, None] + perpendicular(rng, nc) * sin_i[:, None]).astype(F)
    rows = np.arange(n)
    axis = rng.integers(0, 3, n)
    dc[rows, axis] = ulp_step(dc[rows, axis], rng.integers(-2, 3, n))
    nrm[s], d[s] = nc[s], dc.astype(np.float64)[s]

    o = rng.uniform(-1, 1, (n, 3))
    pos = rng.uniform(-1, 1, (n, 3)).astype(F)
    rays = np.concatenate([o, d], axis=1).astype(F)
    return rays, pos, nrm.astype(F), ior, rng_states(rng, n)


# ---- bsdf_spectrum -----------------------------------------------------------------------------------------------------------

def reflect32(v, nrm):
    """reflect() of util/vector.h in float32: v - (n * 2) * dot(v, n), the dot product accumulated from 0 left to right."""
    v, nrm = np.asarray(v, F), np.asarray(nrm, F)
    dot = F(0.0) + v[:, 0] * nrm[:, 0]
    dot = dot + v[:, 1] * nrm[:, 1]
    dot = dot + v[:, 2] * nrm[:, 2]
    return (v - (nrm * F(2.0)) * dot[:, None]).astype(F)


def bsdf_spectrum_family(seed, n=24000):
    """from_dir, to_dir, nrm (n, 3), light, diffuse, specular (n, 4).  Parts: random | to_dir below the horizon | to_dir = reflect(from_dir, n)
    exactly | grazing: dot(n, to_dir) and dot(from_dir, to_dir) exactly 0 and +-denormal | light with zeros and 1e30."""
    rng = np.random.default_rng(seed)
    nrm = random_dirs(rng, n)
    from_dir = random_dirs(rng, n)
    to_dir = random_dirs(rng, n)
    to_dir = np.where((np.sum(to_dir * nrm, axis=1) < 0)[:, None], -to_dir, to_dir)  # above the horizon unless a part says otherwise
    light = rng.uniform(0, 4, (n, 4))
    parts = _parts(n, 5)

    s = parts[1]
    to_dir[s] = -to_dir[s]

    s = parts[2]
    to_dir[s] = reflect32(from_dir, nrm).astype(np.float64)[s]

    s = parts[3]
    i = rng.integers(0, 6, n)
    j = (i // 2 * 2 + 2 + 2 * rng.integers(0, 2, n) + rng.integers(0, 2, n)) % 6
    tiny = rng.choice([0.0, -0.0, 1.4e-45, -1.4e-45, 1e-38, -1e-38], n)[:, None]
    graze_n = rng.random(n) < 0.5  # to_dir in the surface | to_dir perpendicular to from_dir
    to_ax = AXES[j] + AXES[i] * tiny
    nrm[s] = np.where(graze_n[:, None], AXES[i], nrm)[s]
    from_dir[s] = np.where(graze_n[:, None], from_dir, AXES[i])[s]
    general = rng.random(n) < 0.3
    to_gen = perpendicular(rng, np.where(graze_n[:, None], nrm, from_dir))
    to_dir[s] = np.where(general[:, None], to_gen, to_ax)[s]

    s = parts[4]
    special = rng.choice([0.0, 1e30, 1.0, 1e-30], (n, 4))
    light[s] = special[s]

    diffuse = rng.uniform(0, 1, (n, 4))
    specular = rng.uniform(0, 1, (n, 4))
    return from_dir.astype(F), to_dir.astype(F), nrm.astype(F), light.astype(F), diffuse.astype(F), specular.astype(F)


# ---- camera_shoot / camera_shoot_lane ------------------------------------------------------------------------------------------

PIXEL_SIZES = [0.0] + [2.0 / w for w in (1, 37, 1024)]
SENSOR_EDGES = np.array([-1.0, 0.0, 1.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24)], dtype=F)


def camera_cases():
    """name -> camera dict: every aperture kind, aperture sizes 0 and 1e-6 beside an ordinary one, hex_ratio 0, 0.4, 1, with a focal
    plane and with focal_plane_dist = 0."""
    from cpupathtrace_amd import scenes
    cams = {}
    for focal in (0.0, 2.5):
        cams["none_f%g" % focal] = scenes.camera((0.3, 0.2, -2.5), (0, 0.1, 0), (0.1, 1, 0), 0.8, 1.2, 1.6, 0.0, 0.0, scenes.APERTURE_NONE, 0.0, focal)
        for size in (0.0, 1e-6, 0.07):
            cams["circular_a%g_f%g" % (size, focal)] = scenes.camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0, size, size * 0.5,
                                                                     scenes.APERTURE_CIRCULAR, 0.0, focal)
            for ratio in (0.0, 0.4, 1.0):
                cams["hex_a%g_r%g_f%g" % (size, ratio, focal)] = scenes.camera((0.3, 0.2, -2.5), (0, 0.1, 0), (0.1, 1, 0), 0.8, 1.2, 1.6, size, size * 0.4,
                                                                               scenes.APERTURE_HEXAGONAL, ratio, focal)
    return cams


def camera_family(seed, n=512):
    """xy (n, 2), states (n,): sensor positions from {-1, 0, 1, +-(1 - 2^-24)} in either coordinate mixed with random ones."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1, 1, (n, 2)).astype(F)
    edge = rng.random((n, 2)) < 0.5
    xy = np.where(edge, SENSOR_EDGES[rng.integers(0, len(SENSOR_EDGES), (n, 2))], xy).astype(F)
    return xy, rng_states(rng, n)


# ---- engine --------------------------------------------------------------------------------------------------------------------

RNG_SEEDS = [0, 1, U64_MAX]
RNG_DRAWS = 4096
UNIFORM_RANGES = [(0.0, 1.0), (-1.0 / 512.0, 1.0 / 512.0), (-0.25, 1.5), (1.0, float(np.nextafter(F(1.0), F(2.0))))]
BERNOULLI_P = [0.0, 1.0, 0.5, 1e-3, 0.3333333432674408, 1.0 - 2.0 ** -24]


# ---- device libm: input bit patterns ---------------------------------------------------------------------------------------------

def f32_bits(x):
    return int(np.array(x, dtype=F).view(np.uint32))


def window(centre_bits, half=4096, lo=0, hi=0x7F800000):
    """The bit patterns centre - half .. centre + half, clipped to [lo, hi]."""
    return np.arange(max(centre_bits - half, lo), min(centre_bits + half, hi) + 1, dtype=np.int64)


def sincos_inputs(stride=61):
    """Every stride-th float of [0, 7] from bit pattern 0 (subnormals included) and dense windows of +-4096 floats around 0 (both signs),
    the smallest normal, every multiple of pi/4 up to 7 and the two abstop12 thresholds sinf/cosf branch on (2^-12 and pi/4's binade)."""
    top = f32_bits(7.0)
    chunks = [np.arange(0, top + 1, stride, dtype=np.int64), window(0), window(0) | 0x80000000, window(0x00800000)]
    for k in range(1, 9):
        chunks.append(window(f32_bits(k * np.pi / 4), hi=top))
    for thr in (f32_bits(2.0 ** -12), (f32_bits(np.pi / 4) >> 20) << 20):
        chunks.append(window(thr))
    return np.unique(np.concatenate(chunks)).astype(np.uint32)


def acos_inputs(stride=61):
    """Every stride-th float of [-1, 1] and dense windows at +-1 (the NaN side included), +-0.5, 0 and the 2^-26 threshold."""
    one = f32_bits(1.0)
    mag = [np.arange(0, one + 1, stride, dtype=np.int64), window(one), window(f32_bits(0.5)), window(0), window(0x32800000)]
    mag = np.unique(np.concatenate(mag))
    return np.concatenate([mag, mag | 0x80000000]).astype(np.uint32)


POW_EXPONENTS = np.array([0.5, 1.0, 1 / 1.8 - 1, 1 / 2.2 - 1, 9.0, -0.5, 2.0, 3.0, -1.0, 1e-3, 1e3], dtype=F)


def pow_sweep_bases(stride=251):
    """Every stride-th non-negative float, 0 and +inf included."""
    return np.unique(np.concatenate([np.arange(0, 0x7F800000, stride, dtype=np.int64), [0x7F800000]])).astype(np.uint32)


def pow_random_pairs(n=2000000):
    """The random bit pairs of tests/test_abi_cpu.py (xorshift64 from 88172645463325252: low word = base, high word = exponent)."""
    mask = U64_MAX
    state = 88172645463325252
    out = np.empty(n, dtype=np.uint64)
    for i in range(n):
        state ^= (state << 13) & mask
        state ^= state >> 7
        state ^= (state << 17) & mask
        out[i] = state
    return (out & 0xFFFFFFFF).astype(np.uint32), (out >> 32).astype(np.uint32)


def pow_special_pairs(seed=7):
    """Paired (x, y) bit patterns: negative bases with integer, half-integer and huge exponents (the checkint paths); +-0, +-inf and NaN in
    either argument; pairs whose result is subnormal, underflows or overflows."""
    rng = np.random.default_rng(seed)
    inf, nan = np.inf, np.nan
    neg = np.array([-0.5, -1.0, -2.0, -3.5, -1e-40, -1.1754944e-38, -1e30, -3.0, -0.999, -inf, -0.0], dtype=F)
    ys = np.concatenate([np.arange(-6, 7), [0.5, -0.5, 1.5, -1.5, 2.5, 1e-3], [2.0 ** 22 + 0.5, 2.0 ** 23 - 1, 2.0 ** 23 - 0.5, 2.0 ** 23, 2.0 ** 23 + 1],
                         [2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 31, 1e10, -1e10, 3e38, -3e38, 127.0, 128.0, -149.0, -150.0, 1023.0]]).astype(F)
    pairs = [np.stack(np.meshgrid(neg, ys, indexing="ij"), axis=-1).reshape(-1, 2)]
    special = np.array([0.0, -0.0, inf, -inf, nan], dtype=F)
    plain = np.concatenate([special, np.array([1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 3.0, -3.0, 1e-40, -1e-40, 1e30, 0.999, 1.001, 2.5, -2.5], dtype=F)])
    pairs.append(np.stack(np.meshgrid(special, plain, indexing="ij"), axis=-1).reshape(-1, 2))
    pairs.append(np.stack(np.meshgrid(plain, special, indexing="ij"), axis=-1).reshape(-1, 2))
    # results around 2^-126 (subnormal), 2^-150 (underflow) and 2^128 (overflow): y * log2(x) swept across those values
    m = 60000
    x = np.exp2(rng.uniform(-20, 20, m) + np.where(rng.random(m) < 0.5, 0.2, -0.2))
    x = np.where(np.abs(np.log2(x)) < 0.05, 3.0, x).astype(F)
    x[::7] = rng.choice(np.array([2.0, 0.5, 4.0, 10.0, 0.1, 1e-40, 1e-44, 1e38], dtype=F), len(x[::7]))
    x[3::11] *= F(-1.0)  # (negative bases reach these paths through an odd-integer exponent only; most of these are NaN on both sides)
    want = np.concatenate([rng.uniform(-152, -124, m // 2), rng.uniform(125, 130, m - m // 2)])
    rng.shuffle(want)
    y = (want / np.log2(np.abs(x.astype(np.float64)))).astype(F)
    whole = rng.random(m) < 0.3  # whole-number exponents keep a negative base real
    y = np.where(whole, np.round(y), y).astype(F)
    pairs.append(np.stack([x, y], axis=-1))
    p = np.concatenate(pairs).astype(F)
    return np.ascontiguousarray(p[:, 0]).view(np.uint32), np.ascontiguousarray(p[:, 1]).view(np.uint32)


def pow_unit_bases(stride=61):
    """powf_glibc's domain on the path: every stride-th float of [2^-33, 1], and 0."""
    return np.unique(np.concatenate([[0], np.arange(f32_bits(2.0 ** -33), f32_bits(1.0) + 1, stride, dtype=np.int64), [f32_bits(1.0)]])).astype(np.uint32)


# ---- what a family must contain ------------------------------------------------------------------------------------------------

SLAB_WALK_NAN_CAP = 0.05


def assert_hits_and_misses(t, what):
    """A hit/miss family must hold at least 10 % hits and 10 % misses by the reference's own answer, or bit-equality on it proves little."""
    hits = float((np.asarray(t) >= 0).mean())
    assert 0.10 <= hits <= 0.90, "%s: %.1f %% hits" % (what, 100 * hits)


def assert_slab_walk_exclusion(mask):
    share = float(np.asarray(mask).mean())
    assert 0.0 < share < SLAB_WALK_NAN_CAP, "slab_walk: %.2f %% of the family has a NaN product" % (100 * share)
