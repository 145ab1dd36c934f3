"""Nearest-surface queries without a GPU (include/pt_nearest.h): the numpy restatement (tests/nearest_ref.py) on
hand-made cases with known answers and against an independent float64 formulation; the pruning rule's margin re-measured on families of
(point, triangle) and (point, sphere) pairs; the device functions compiled for the host (tests/hip/nearest_probe.hip) against the
restatement, bit for bit; the record's format; the exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cpupathtrace_amd import binding, build
from tests import nearest_probe, nearest_ref as ref, pose_probe, query_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
EPS = 2.0 ** -23
N_PAIRS = 20000
# The float64 agreement: |restated distance - float64 distance| in units of eps * M over the families below.  Measured worst case 2.06
# (family "on box planes"; 1.40 .. 1.70 on unit, far and slivers, below 0.02 on the offset families, whose errors scale with the
# distance and not with M); the bound is that with a margin of 4.
AGREEMENT_BOUND = 4 * 2.06


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return nearest_probe.Probe(nearest_probe.build_host(str(tmp_path_factory.mktemp("nearest_probe") / "libnearest_probe.so")))


@pytest.fixture(scope="module")
def assembler(tmp_path_factory):
    return pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("nearest_pose") / "libpose_probe.so")))


def families(seed=5):
    """{name: (p, a, b, c)} float32, N_PAIRS rows each: unit scale; far points; coordinates offset by 1e3 and by 1e5; slivers; points
    exactly on the planes of the triangle's box.  Every family also holds points close to its triangles."""
    rng = np.random.default_rng(seed)
    out = {}

    def tris(scale, offset):
        a = rng.normal(size=(N_PAIRS, 3)) * scale + offset
        return a.astype(F), (a + rng.normal(size=(N_PAIRS, 3)) * scale).astype(F), (a + rng.normal(size=(N_PAIRS, 3)) * scale).astype(F)

    def near(a, spread):
        p = a + rng.normal(size=a.shape) * spread
        p[::4] = a[::4] + rng.normal(size=a[::4].shape) * spread * 1e-2
        return p.astype(F)

    a, b, c = tris(1.0, 0.0)
    out["unit"] = (near(a, 3.0), a, b, c)
    a, b, c = tris(1.0, 0.0)
    out["far"] = ((a + rng.normal(size=a.shape) * 1e3).astype(F), a, b, c)
    a, b, c = tris(1.0, 1e3)
    out["offset 1e3"] = (near(a, 3.0), a, b, c)
    a, b, c = tris(1.0, 1e5)
    out["offset 1e5"] = (near(a, 3.0), a, b, c)
    a, b, _ = tris(1.0, 0.0)
    c = (a + (b - a) * rng.random((N_PAIRS, 1)) + rng.normal(size=a.shape) * 1e-3).astype(F)
    out["slivers"] = (near(a, 3.0), a, b, c)
    a, b, c = tris(1.0, 0.0)
    p = near(a, 3.0)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    axis = rng.integers(0, 3, N_PAIRS)
    rows = np.arange(N_PAIRS)
    p[rows, axis] = np.where(rng.random(N_PAIRS) < 0.5, lo[rows, axis], hi[rows, axis])
    out["on box planes"] = (p, a, b, c)
    return out


def sphere_families(seed=6):
    rng = np.random.default_rng(seed)
    out = {}
    for name, offset, spread in (("unit", 0.0, 3.0), ("far", 0.0, 1e3), ("offset 1e3", 1e3, 3.0), ("offset 1e5", 1e5, 3.0)):
        c = (rng.normal(size=(N_PAIRS, 3)) + offset).astype(F)
        radius = rng.uniform(0.05, 2.0, N_PAIRS).astype(F)
        p = (c + rng.normal(size=c.shape) * spread).astype(F)
        p[::5] = (c[::5] + rng.normal(size=c[::5].shape) * 1e-3).astype(F)
        out[name] = (p, c, radius)
    return out


def degenerate(seed=7):
    """Triangles with two or three equal corners, collinear corners and a zero edge, each with points around them."""
    rng = np.random.default_rng(seed)
    n = 600
    a = rng.normal(size=(n, 3)).astype(F)
    b = (a + rng.normal(size=(n, 3))).astype(F)
    c = (a + rng.normal(size=(n, 3))).astype(F)
    k = np.arange(n) % 5
    b = np.where((k == 0)[:, None] | (k == 3)[:, None], a, b)                      # a == b; a == b == c
    c = np.where((k == 1)[:, None], a, np.where((k == 2)[:, None], b, c))          # a == c; b == c
    c = np.where((k == 3)[:, None], a, c)
    c = np.where((k == 4)[:, None], (a + (b - a) * F(2.0)).astype(F), c).astype(F)  # collinear
    p = (a + rng.normal(size=(n, 3))).astype(F)
    return p, a, b.astype(F), c


def edges(a, b, c):
    return (b - a).astype(F), (c - a).astype(F)


# ---- 1. the restatement on cases with known answers ---------------------------------------------------------------------------------------------------

A, B, Cc = np.array([0, 0, 0], F), np.array([1, 0, 0], F), np.array([0, 1, 0], F)
HAND = [((0.25, 0.25, 1.0), 0, 1.0, (0.25, 0.25, 0.0), 0.25, 0.25), ((0.5, -1.0, 0.0), 1, 1.0, (0.5, 0.0, 0.0), 0.5, 0.0),
        ((1.0, 1.0, 0.0), 2, np.sqrt(0.5), (0.5, 0.5, 0.0), 0.5, 0.5), ((-1.0, 0.5, 0.0), 3, 1.0, (0.0, 0.5, 0.0), 0.0, 0.5),
        ((-1.0, -1.0, 0.0), 4, np.sqrt(2.0), (0.0, 0.0, 0.0), 0.0, 0.0), ((2.0, -0.5, 0.0), 5, np.sqrt(1.25), (1.0, 0.0, 0.0), 1.0, 0.0),
        ((-0.5, 2.0, 0.0), 6, np.sqrt(1.25), (0.0, 1.0, 0.0), 0.0, 1.0)]


def hand_scene():
    """One triangle (object 0) and, far from it, one sphere of radius 1 around (10, 0, 0) (object 1)."""
    scene = dict(obj_kind=np.array([0, 1], np.uint8), tri_pos=np.concatenate([A, B, Cc]).reshape(1, 9), tri_nrm=np.tile(np.array([0, 0, 1], F), 3).reshape(1, 9),
                 tri_cull=np.zeros(1, np.uint8), tri_material=np.array([3], np.uint32), sph=np.array([[10.0, 0.0, 0.0, 1.0]], F), sph_material=np.array([5], np.uint32))
    return dict(scene=scene, first=np.zeros(0, np.int64), count=np.zeros(0, np.int64), n_faces=[], face_first=[], face_of=np.zeros(0, np.uint32), n_desc=2)


def test_every_feature_code_on_hand_made_cases(probe):
    flat = hand_scene()
    points = [h[0] for h in HAND] + [(12.0, 0.0, 0.0), (10.5, 0.0, 0.0), (10.0, 0.0, 0.0)]
    got = ref.records(flat, points)
    for rec, (_, feature, distance, position, b1, b2) in zip(got, HAND):
        assert rec["feature"] == feature and rec["object"] == 0 and rec["material"] == 3 and rec["instance"] == -1 and rec["face"] == ref.query_ref.NO_FACE
        assert abs(rec["distance"] - distance) < 1e-6 and abs(rec["squared_distance"] - distance ** 2) < 1e-6
        assert np.allclose(rec["position"], position, atol=1e-6) and abs(rec["b1"] - b1) < 1e-6 and abs(rec["b2"] - b2) < 1e-6
        assert rec["geometric_normal"].tolist() == [0.0, 0.0, 1.0]
    assert got["side"][:7].tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert ref.records(flat, [(0.25, 0.25, -1.0)])["side"][0] == -1
    outside, inside, centre = got[7], got[8], got[9]
    for rec, distance, side in ((outside, 1.0, 1), (inside, 0.5, -1), (centre, 1.0, -1)):
        assert rec["feature"] == 7 and rec["object"] == 1 and rec["material"] == 5 and rec["b1"] == 0 and rec["b2"] == 0
        assert rec["distance"] == F(distance) and rec["squared_distance"] == F(distance * distance) and rec["side"] == side
        assert rec["position"].tolist() == [11.0, 0.0, 0.0] and rec["geometric_normal"].tolist() == [1.0, 0.0, 0.0]
    assert sorted(set(got["feature"].tolist())) == list(range(8))
    # the definition's thresholds: in range iff d2 <= r * r; a miss otherwise, for a NaN or negative r, a NaN coordinate, an empty scene
    r = got["distance"].copy()
    in_range = ref.records(flat, points, r)
    with np.errstate(all="ignore"):
        want = got["squared_distance"] <= (r * r).astype(F)
    assert (in_range["object"][want] == got["object"][want]).all() and (in_range["object"][~want] == -1).all()
    for bad in (-1.0, np.nan, 0.0):
        ref.assert_records_equal(ref.records(flat, points, bad), ref.miss(len(points)), "r = %r" % bad)
    ref.assert_records_equal(ref.records(flat, [(np.nan, 0, 0), (0, np.nan, 0), (0, 0, np.nan)]), ref.miss(3), "NaN coordinates")
    ref.assert_records_equal(ref.records(flat, [(np.inf, 0, 0)], 1e10), ref.miss(1), "an infinite coordinate, a finite range")
    assert ref.records(flat, [(0.0, 0.0, 0.0)], 0.0)["object"][0] == 0  # distance 0 is within r = 0
    empty = dict(hand_scene(), scene=dict(obj_kind=np.zeros(0, np.uint8), tri_pos=np.zeros((0, 9), F), tri_nrm=np.zeros((0, 9), F), tri_cull=np.zeros(0, np.uint8),
                                          tri_material=np.zeros(0, np.uint32), sph=np.zeros((0, 4), F), sph_material=np.zeros(0, np.uint32)), n_desc=0)
    ref.assert_records_equal(ref.records(empty, points), ref.miss(len(points)), "an empty scene")
    # the host compile of the device's record agrees on all of it
    ref.assert_records_equal(probe.records(flat, points), got, "hand-made cases, host compile")
    ref.assert_records_equal(probe.records(flat, points, r), in_range, "hand-made cases at their own distance, host compile")


def test_the_restatement_agrees_with_an_independent_float64_formulation():
    worst = {}
    for name, (p, a, b, c) in families().items():
        ab, ac = edges(a, b, c)
        d2 = ref.triangle(p, a, ab, ac)[0]
        assert not np.isnan(d2).any(), name
        m = np.maximum(np.abs(p).max(axis=1), np.maximum(np.abs(a).max(axis=1), np.maximum(np.abs(b).max(axis=1), np.abs(c).max(axis=1)))).astype(D)
        err = np.abs(np.sqrt(d2.astype(D)) - ref.triangle_distance64(p, a, b, c)) / (EPS * m)
        worst[name] = float(err.max())
        print("float64 agreement, %-14s worst %.2f eps*M" % (name + ":", worst[name]))
    assert max(worst.values()) <= AGREEMENT_BOUND, worst


# ---- 2. the pruning margin ----------------------------------------------------------------------------------------------------------------------------

def test_the_margin_covers_the_plain_bounds_shortfall_fourfold():
    """On every family: the margin-reduced bound of the object's own box never exceeds the restated d2; the plain bound does, somewhere
    -- that is why the margin exists --, and m = M * 2^-18 (32 ulp of M) is at least four times its worst shortfall."""
    worst_ulp, failures = 0.0, 0
    for kind, fams in (("triangle", families()), ("sphere", sphere_families())):
        for name, pair in fams.items():
            if kind == "triangle":
                p, a, b, c = pair
                d2 = ref.triangle(p, a, *edges(a, b, c))[0]
                lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
            else:
                p, centre, radius = pair
                d2 = ref.sphere(p, centre, radius)[0]
                lo, hi = (centre - radius[:, None]).astype(F), (centre + radius[:, None]).astype(F)
            big = np.maximum(np.abs(p).max(axis=1), np.maximum(np.abs(lo).max(axis=1), np.abs(hi).max(axis=1))).astype(F)  # (the root box is at least this one: M only grows)
            bound = ref.box_bound(p, lo, hi, (big * ref.MARGIN).astype(F))
            assert (bound <= d2).all(), (kind, name, int((bound > d2).sum()))
            plain = ref.plain_bound(p, lo, hi)
            short = plain > d2
            ulp = np.where(short, (np.sqrt(plain.astype(D)) - np.sqrt(d2.astype(D))) / (big.astype(D) * EPS), 0.0)
            kept = ((bound > 0) & (plain > 0)).sum() / max((plain > 0).sum(), 1)
            print("margin, %-8s %-14s plain bound above d2 for %5.2f %% of the pairs, worst shortfall %.2f ulp of M; the rule keeps a positive bound for %.1f %% of them" % (
                kind, name + ":", 100.0 * short.mean(), float(ulp.max()), 100.0 * kept))
            worst_ulp, failures = max(worst_ulp, float(ulp.max())), failures + int(short.sum())
    print("margin: worst shortfall of the plain bound %.2f ulp of M; m is 32 ulp of M" % worst_ulp)
    assert failures > 0, "the plain bound never failed: the families do not show why the margin exists"
    assert float(ref.MARGIN) / EPS >= 4.0 * worst_ulp, worst_ulp


# ---- 3. the device functions, compiled for the host ---------------------------------------------------------------------------------------------------

def bits_equal(got, want, what):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    assert not bad.any(), "%s: %d of %d differ, first at %s: got %r want %r" % (what, bad.sum(), bad.size, np.argwhere(bad)[0].tolist(), g[bad][0], w[bad][0])


def test_the_host_compile_equals_the_restatement_bit_for_bit(probe):
    fams = dict(families(), degenerate=degenerate())
    for name, (p, a, b, c) in fams.items():
        ab, ac = edges(a, b, c)
        want = ref.triangle(p, a, ab, ac)
        got = probe.triangles(p, a, ab, ac)
        for k, field in enumerate(("d2", "v", "w")):
            bits_equal(got[k], want[k], "%s: %s" % (name, field))
        assert (got[3] == want[3]).all(), name
        bits_equal(got[4], want[4], "%s: diff" % name)
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        root_lo, root_hi = lo.min(axis=0), hi.max(axis=0)
        m = (ref.magnitude(p, root_lo, root_hi) * ref.MARGIN).astype(F)
        bits_equal(probe.margins(p, root_lo, root_hi), m, "%s: margin" % name)
        bits_equal(probe.bounds(p, lo, hi, m), ref.box_bound(p, lo, hi, m), "%s: bound" % name)
    p, a, b, c = fams["degenerate"]
    assert np.isnan(ref.triangle(p, a, *edges(a, b, c))[0]).any(), "the degenerate family has no NaN d2"
    for name, (p, c, radius) in sphere_families().items():
        want = ref.sphere(p, c, radius)
        got = probe.spheres(p, np.concatenate([c, radius[:, None]], axis=1))
        bits_equal(got[0], want[0], "sphere %s: d2" % name)
        bits_equal(got[1], want[2], "sphere %s: len" % name)
        bits_equal(got[2], want[3], "sphere %s: dist" % name)
        assert (got[3] == 7).all()


def test_a_nan_distance_is_never_chosen(probe):
    """A scene of the degenerate triangles and one far sphere: every query has an answer, its d2 is not NaN, and both the restatement and
    the host compile give it -- in any order of the leaves."""
    p, a, b, c = degenerate()
    n = len(a)
    scene = dict(obj_kind=np.concatenate([np.zeros(n, np.uint8), np.ones(1, np.uint8)]), tri_pos=np.concatenate([a, b, c], axis=1), tri_nrm=np.tile(np.array([0, 0, 1], F), (n, 3)),
                 tri_cull=np.zeros(n, np.uint8), tri_material=np.arange(n, dtype=np.uint32), sph=np.array([[50.0, 0.0, 0.0, 1.0]], F), sph_material=np.array([7], np.uint32))
    flat = dict(hand_scene(), scene=scene, n_desc=n + 1)
    d2 = ref.all_d2(scene, p)
    assert np.isnan(d2).any() and np.isnan(d2).all(axis=1).sum() == 0
    want = ref.records(flat, p)
    assert (want["object"] >= 0).all() and not np.isnan(want["squared_distance"]).any()
    ref.assert_records_equal(probe.records(flat, p), want, "degenerate triangles")
    order = np.concatenate([np.arange(n), [n + 1]])
    ref.assert_records_equal(probe.records(flat, p, order=order[::-1]), want, "degenerate triangles, leaves in descending order")


def points_of(flat, n, seed):
    """Points around scene S and on it: in 1.5x its box, and corners of its triangles (exact ties between neighbours)."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(flat["scene"]["tri_pos"], F).reshape(-1, 3, 3)
    lo, hi = tri.reshape(-1, 3).min(axis=0), tri.reshape(-1, 3).max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.75 * (hi - lo)
    free = rng.uniform(mid - half, mid + half, (n - n // 3, 3))
    return np.concatenate([free, tri[rng.integers(0, len(tri), n // 3), rng.integers(0, 3, n // 3)]]).astype(F)


def test_records_of_scene_s_by_the_host_compile(probe, assembler):
    """The whole record -- object, instance, face by both rules, material, normals, side -- on scene S, restatement against host compile,
    unbounded and at a threshold, leaves in three orders: ties go to the lowest record index whatever the order."""
    scene, instances, shapes = cases.build(False)
    flat = cases.flatten(scene, instances, shapes, assembler)
    p = points_of(flat, 300, 11)
    want, ties = ref.records(flat, p, want_ties=True)
    assert (ties >= 2).sum() >= 50 and (want["instance"] >= 0).any() and (want["instance"] < 0).any() and (want["feature"] == 7).any()
    n_tris = len(np.asarray(flat["scene"]["tri_pos"]).reshape(-1, 9))
    order = np.concatenate([np.arange(n_tris), n_tris + 1 + np.arange(2)])
    for what, o in (("ascending", order), ("descending", order[::-1]), ("shuffled", np.random.default_rng(3).permutation(order))):
        ref.assert_records_equal(probe.records(flat, p, order=o), want, "scene S, leaves " + what)
    ref.assert_records_equal(probe.records(flat, p, with_table=True), ref.records(flat, p, with_table=True), "scene S with the face table")
    r = np.full(len(p), np.median(want["distance"]), F)
    limited = ref.records(flat, p, r)
    assert 0.3 <= (limited["object"] >= 0).mean() <= 0.7
    ref.assert_records_equal(probe.records(flat, p, r), limited, "scene S at the median distance")


# ---- 4. the format and the exports ----------------------------------------------------------------------------------------------------------------------

def test_format_and_exports(probe):
    record, grid, offsets = probe.sizes()
    names = ("distance", "object", "instance", "face", "position", "material", "geometric_normal", "b1", "squared_distance", "feature", "side", "b2")
    assert record == 64 == binding.Nearest.itemsize and grid == 36 == binding.DistanceGrid.itemsize
    assert offsets == [binding.Nearest.fields[n][1] for n in names] == [0, 4, 8, 12, 16, 28, 32, 44, 48, 52, 56, 60]
    assert [binding.DistanceGrid.fields[n][1] for n in ("origin", "step", "count")] == [0, 12, 24]
    header = open(os.path.join(ROOT, "include", "pt_nearest.h")).read()
    declared = set(re.findall(r"^int (pt_[a-z_0-9]+)\(", header, re.M))
    assert declared == set(binding.NEAREST_EXPORTS) and len(binding.NEAREST_EXPORTS) == 4
    for name in dir(binding):
        if name.endswith("EXPORTS") and name != "NEAREST_EXPORTS":
            assert not set(getattr(binding, name)) & declared, name
    for k, name in enumerate(("FACE", "EDGE_AB", "EDGE_BC", "EDGE_CA", "VERTEX_A", "VERTEX_B", "VERTEX_C", "SPHERE")):
        assert re.search(r"^#define PT_NEAREST_%s\s+%du$" % (name, k), header, re.M) and getattr(binding, "NEAREST_" + name) == k
    flat = " ".join(header.replace(" * ", " ").split())
    for text in ("robust inside/outside test", "k nearest", "restricted to one instance", "signed grids"):
        assert text in flat[flat.index("Left out:"):], text
    assert '#include "pt_nearest.h"' in open(os.path.join(ROOT, "include", "pt_query.h")).read()
    assert "pt_nearest.cpp" in build.SOURCES and "pt_nearest.hip" in build.SOURCES and "pt_nearest_kernels.h" in build.HEADERS
    assert any(h.endswith(os.path.join("include", "pt_nearest.h")) for h in build.HEADERS)
    lib = C.CDLL(build.build())
    for name in binding.NEAREST_EXPORTS:
        assert hasattr(lib, name), name


def test_refusals_that_need_no_device():
    lib = binding.load()
    pts, recs, dist, obj = np.zeros((2, 4), F), np.zeros(2, binding.Nearest), np.zeros(8, F), np.zeros(8, np.int32)
    grid, zero = binding.distance_grid((0, 0, 0), (1, 1, 1), (2, 2, 2)), binding.distance_grid((0, 0, 0), (1, 1, 1), (2, 0, 2))
    p, n2, inf = binding._ptr, C.c_size_t(2), C.c_float(np.inf)
    calls = [lambda: lib.pt_nearest_points(None, p(pts), n2, p(recs)), lambda: lib.pt_nearest_points_device(None, p(pts), n2, p(recs), None),
             lambda: lib.pt_nearest_points(None, None, C.c_size_t(0), None), lambda: lib.pt_distance_grid_fill(None, p(grid), inf, p(dist), p(obj)),
             lambda: lib.pt_distance_grid_fill_device(None, p(grid), inf, p(dist), None, None), lambda: lib.pt_distance_grid_fill(None, p(zero), inf, p(dist), p(obj))]
    for call in calls:
        assert call() == 1 and b"null" in lib.pt_last_error()  # PT_ERR_INVALID
