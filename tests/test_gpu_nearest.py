"""Nearest-surface queries on the GPU (include/pt_nearest.h): Scene.nearest equals the numpy restatement of the
definition (tests/nearest_ref.py: brute force over every object) bit for bit in every field, at every batch size, unbounded and under
thresholds; distance grids are the same queries at positions made on the device; the device forms write what the host forms return;
after a pose, a deformation, a morph and a relight every record is what a freshly created scene answers; and the calls leave a live
frame as it was.  Scenes S (tree in LDS for the ray walks; host-built) and L (device-built tree, records in HBM, the sliver row that
drives a walk's stack past its LDS window) of tests/query_cases.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cpupathtrace_amd import binding, scenes
from tests import motion_shapes_cases as msc
from tests import nearest_ref as ref, pose_probe, query_cases as cases
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N_POINTS = 1000
_cache = {}


@pytest.fixture(scope="module")
def assembler(tmp_path_factory):
    return pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("nearest_pose") / "libpose_probe.so")))


def root_box(scene):
    tri = np.asarray(scene["tri_pos"], F).reshape(-1, 3)
    sph = np.asarray(scene["sph"], F).reshape(-1, 4)
    lo = np.minimum(tri.min(axis=0), (sph[:, :3] - sph[:, 3:]).min(axis=0))
    hi = np.maximum(tri.max(axis=0), (sph[:, :3] + sph[:, 3:]).max(axis=0))
    return lo.astype(F), hi.astype(F)


def query_points(g, flat, seed=31):
    """N_POINTS points: drawn in 1.5x the root box; positions Scene.query returns (distance about 0); vertices of mesh M1's instances
    exactly as pt_scene_get_triangles returns them; midpoints of shared edges; points 1e3 away; points along the sliver row's axis;
    points that share a coordinate with the root box's planes; points at, in and around the spheres."""
    rng = np.random.default_rng(seed)
    sc = flat["scene"]
    lo, hi = root_box(sc)
    mid, half = 0.5 * (lo + hi), 0.75 * (hi - lo)
    parts = [rng.uniform(mid - half, mid + half, (330, 3))]
    hits = g.query(cases.rays(flat))
    parts.append(hits["position"][hits["object"] >= 0][:150])
    first, count = g.instance_ranges()
    m1 = g.triangles(int(first[0]), int(count[0] + count[1]))[0].reshape(-1, 3, 3)
    pick = rng.integers(0, len(m1), 180)
    parts.append(m1[pick, rng.integers(0, 3, 180)])
    pick = rng.integers(0, len(m1), 120)
    k = rng.integers(0, 3, 120)
    parts.append((F(0.5) * (m1[pick, k] + m1[pick, (k + 1) % 3])).astype(F))
    far = rng.normal(size=(50, 3))
    parts.append(mid + 1e3 * far / np.linalg.norm(far, axis=1, keepdims=True))
    parts.append(np.stack([rng.uniform(-1.1, 1.1, 70), rng.uniform(-0.9, 0.9, 70), rng.uniform(1.55, 1.95, 70)], axis=1))
    on = rng.uniform(mid - half, mid + half, (60, 3))
    axis, rows = rng.integers(0, 3, 60), np.arange(60)
    on[rows, axis] = np.where(rng.random(60) < 0.5, lo[axis], hi[axis])
    parts.append(on)
    sph = np.asarray(sc["sph"], F).reshape(-1, 4)
    around = np.repeat(sph[:, :3], 19, axis=0) + rng.normal(size=(19 * len(sph), 3)) * np.repeat(sph[:, 3:], 19, axis=0) * 0.8
    parts += [sph[:, :3], around]
    p = np.concatenate([np.asarray(x, F) for x in parts]).astype(F)
    assert len(p) == N_POINTS, len(p)
    return np.ascontiguousarray(p[rng.permutation(len(p))])


def load_case(name, assembler):
    """A scene on the device and flattened, its query points, and the restated records of all of them (computed once)."""
    if name not in _cache:
        scene, instances, shapes = cases.build(name == "L")
        flat = cases.flatten(scene, instances, shapes, assembler)
        g = binding.Scene(scene)
        points = query_points(g, flat)
        want, ties = ref.records(flat, points, want_ties=True)
        _cache[name] = dict(name=name, flat=flat, g=g, points=points, want=want, ties=ties)
    return _cache[name]


@pytest.fixture(scope="module", params=["S", "L"])
def case(request, assembler):
    return load_case(request.param, assembler)


def test_the_query_set_meets_its_conditions(case):
    """Checked on the restatement, before the device is compared: ties and every feature code."""
    want, ties = case["want"], case["ties"]
    assert (ties >= 2).sum() >= 100, (ties >= 2).sum()
    assert sorted(set(want["feature"][want["object"] >= 0].tolist())) == list(range(8))
    assert (want["object"] >= 0).all() and (want["distance"] == 0).sum() >= 100 and (want["distance"] > 100).sum() >= 50
    print("%s: %d queries, %d with ties, features %s" % (case["name"], len(want), (ties >= 2).sum(), np.bincount(want["feature"], minlength=8).tolist()))


def test_nearest_is_the_restatement_bit_for_bit(case):
    g, points, want = case["g"], case["points"], case["want"]
    info = g.info()
    if case["name"] == "L":
        assert g.n_objects >= 1024 and info["depth"] > 10, (g.n_objects, info)
    for n in cases.BATCHES:
        ref.assert_records_equal(g.nearest(points[:n]), want[:n], "%s, %d points" % (case["name"], n))
    assert len(g.nearest(np.zeros((0, 3), F))) == 0
    ref.assert_records_equal(g.nearest(points, np.inf), want, "+inf is unbounded")


def test_max_distance(case):
    g, points, want, flat = case["g"], case["points"], case["want"], case["flat"]
    n = len(points)
    miss = ref.miss(n)
    # a per-query threshold at the median distance
    r = np.full(n, np.median(want["distance"]), F)
    got = g.nearest(points, r)
    inside = got["object"] >= 0
    assert 0.3 <= inside.mean() <= 0.7, inside.mean()
    ref.assert_records_equal(got[inside], want[inside], "in range")
    ref.assert_records_equal(got[~inside], miss[~inside], "out of range")
    ref.assert_records_equal(got, ref.records(flat, points, r), "the median threshold against the restatement")
    # r equal to the exact distance: in range only when r * r >= d2
    r = want["distance"].copy()
    got = g.nearest(points, r)
    with np.errstate(all="ignore"):
        keeps = (r * r).astype(F) >= want["squared_distance"]
    assert keeps.any() and (got["object"][keeps] == want["object"][keeps]).all() and (got["object"][~keeps] == -1).all()
    print("%s: r = distance keeps %d of %d queries" % (case["name"], keeps.sum(), n))
    ref.assert_records_equal(got, ref.records(flat, points, r), "r = distance against the restatement")
    # 0 keeps the queries at distance 0 alone; negative and NaN thresholds are misses
    got = g.nearest(points, 0.0)
    zero = want["squared_distance"] == 0
    assert zero.sum() >= 100
    ref.assert_records_equal(got[zero], want[zero], "r = 0 at distance 0")
    ref.assert_records_equal(got[~zero], miss[~zero], "r = 0 elsewhere")
    for bad in (-1.0, -np.inf, np.nan):
        ref.assert_records_equal(g.nearest(points[:130], bad), miss[:130], "r = %r" % bad)
    mixed = np.where(np.arange(n) % 3 == 0, F(np.nan), np.where(np.arange(n) % 3 == 1, F(-0.5), F(np.inf))).astype(F)
    ref.assert_records_equal(g.nearest(points, mixed), ref.records(flat, points, mixed), "NaN, negative and infinite thresholds side by side")
    # NaN and infinite coordinates: a NaN is a miss whatever r; an infinite one is a miss for every r whose square is finite, and what
    # the definition says otherwise
    odd = points[:12].copy()
    odd[0:3, 0], odd[3:6, 1], odd[6:9, 2] = np.nan, np.inf, -np.inf
    odd[9] = np.nan
    odd[10] = np.inf
    ref.assert_records_equal(g.nearest(odd[:11], 1e10), miss[:11], "NaN and infinite coordinates")
    got = g.nearest(odd)
    ref.assert_records_equal(got, ref.records(flat, odd), "NaN and infinite coordinates, unbounded")
    assert (got["object"][[0, 1, 2, 9]] == -1).all() and got["object"][11] >= 0


def test_a_single_object_and_an_empty_scene():
    sb = scenes.SceneBuilder()
    sb.triangles([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    points = np.array([[0.25, 0.25, 1.0], [2.0, -0.5, 0.0], [0.5, -1.0, 0.0], [0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]], F)
    g = binding.Scene(sb.build())
    try:
        got = g.nearest(points)
        assert got["object"].tolist() == [0, 0, 0, 0, -1] and got["feature"][:4].tolist() == [0, 5, 1, 4] and got["side"].tolist() == [1, 0, 0, 0, 0]
        assert got["distance"][:4].tolist() == [1.0, float(np.sqrt(F(1.25))), 1.0, 0.0] and (got["instance"] == -1).all()
        assert g.nearest(points, 0.5)["object"].tolist() == [-1, -1, -1, 0, -1]
        distance, obj = g.distance_grid((0.25, 0.25, -1.0), (1.0, 1.0, 1.0), (1, 1, 3))
        assert distance.ravel().tolist() == [1.0, 0.0, 1.0] and obj.ravel().tolist() == [0, 0, 0]
    finally:
        g.close()
    g = binding.Scene(scenes.empty_scene()[0])
    try:
        ref.assert_records_equal(g.nearest(points), ref.miss(len(points)), "an empty scene")
        distance, obj = g.distance_grid((0, 0, 0), (1, 1, 1), (3, 2, 2))
        assert np.isinf(distance).all() and (distance > 0).all() and (obj == -1).all()
    finally:
        g.close()


def test_distance_grid_is_nearest_at_the_stated_positions(case):
    g, flat = case["g"], case["flat"]
    lo, hi = root_box(flat["scene"])
    count = (9, 7, 5)
    origin = (lo - F(0.1)).astype(F)
    step = ((hi - lo + F(0.2)) / (np.asarray(count, F) - F(1.0))).astype(F)
    iz, iy, ix = np.meshgrid(np.arange(5), np.arange(7), np.arange(9), indexing="ij")
    index = np.stack([ix, iy, iz], axis=-1).astype(F)
    positions = (origin + (index * step).astype(F)).astype(F).reshape(-1, 3)  # one product and one sum per axis
    for r in (np.inf, 0.2):
        want = g.nearest(positions, r)
        distance, obj = g.distance_grid(origin, step, count, r)
        assert distance.shape == (5, 7, 9) and obj.shape == (5, 7, 9) and distance.dtype == F and obj.dtype == np.int32
        assert_bits_equal(distance.ravel(), want["distance"], "grid distance, r = %r" % r)
        assert (obj.ravel() == want["object"]).all()
        alone, none = g.distance_grid(origin, step, count, r, want_object=False)
        assert none is None
        assert_bits_equal(alone, distance, "without out_object")
        ref.assert_records_equal(want, ref.records(flat, positions, r), "the grid's positions against the restatement")
    assert np.isinf(distance).any() and (obj == -1).any() and (obj >= 0).any()


def test_instances_and_faces_follow_the_ranges_and_the_face_table(case):
    g, points, flat, want = case["g"], case["points"], case["flat"], case["want"]
    first, count = g.instance_ranges()
    got = g.nearest(points)
    obj = got["object"].astype(np.int64)
    want_instance = np.full(len(obj), -1)
    for i in range(len(first)):
        want_instance[(obj >= int(first[i])) & (obj < int(first[i]) + int(count[i]))] = i
    assert (got["instance"] == want_instance).all() and len(np.unique(want_instance)) == len(first) + 1
    m1, m2 = (got["instance"] == 0) | (got["instance"] == 1), got["instance"] == 2
    assert m1.any() and (got["face"][m1] == (obj - first[got["instance"]])[m1]).all()   # an instance that kept every face
    assert m2.any() and (got["face"][m2] == binding.QUERY_NO_FACE).all()                 # no table yet
    matrices = g.pose_transforms()
    g.mark_motion()
    try:
        ref.assert_records_equal(g.nearest(points), want, "a mark alone")
        g.pose(matrices)  # (the same pose: the rebuild makes the table, and a tree of its own)
        marked = g.nearest(points)
        assert (marked["face"][m2] == flat["local_face"][obj[m2] - flat["n_desc"]]).all() and (marked["face"][m2] < 40).all()
        ref.assert_records_equal(marked, ref.records(flat, points, with_table=True), "with the table")
    finally:
        g.unmark_motion()
    ref.assert_records_equal(g.nearest(points), want, "after the mark is gone")


MORPHS = [(None, np.stack([np.zeros(49, F), 0.05 * msc.patch()[0][:, 0], 0.12 * msc.patch()[0][:, 1]], axis=1).astype(F))]


def test_nearest_follows_the_scene_in_place(assembler):
    """Scene S through a pose, a deformation, a morph and a relight: after each, every record and the grid equal those of a scene created
    afresh in the new state."""
    case = load_case("S", assembler)
    points = case["points"]
    scene, instances, _ = cases.build(False)
    g = binding.Scene(scene)
    state = dict(matrices=[m for _, m, _, _, _ in instances], meshes={}, materials={}, instance_materials={})
    grid = ((-1.0, -1.0, 0.0), (0.25, 0.25, 0.25), (9, 9, 8))
    try:
        def step(what):
            fresh_scene, _, _ = cases.build(False, **state)
            fresh = binding.Scene(fresh_scene)
            try:
                want, got = fresh.nearest(points), g.nearest(points)
                ref.assert_records_equal(got, want, what)
                for a, b in zip(g.distance_grid(*grid), fresh.distance_grid(*grid)):
                    assert a.tobytes() == b.tobytes(), what
                return want
            finally:
                fresh.close()

        before = step("as created")
        ref.assert_records_equal(before, case["want"], "as created, against the restatement")
        state["matrices"][0] = msc.place(-0.4, -0.3, 0.55, 0.75, degrees=12.0)
        state["matrices"][2] = msc.place(0.05, 0.0, 1.0, 1.1, degrees=5.0)
        g.pose([state["matrices"][0], state["matrices"][2]], instances=[0, 2])
        posed = step("posed")
        assert not (posed["distance"] == before["distance"]).all()
        g.deform(vertices={0: msc.patch_bent(0.15)})
        state["meshes"] = {"m1": g.mesh_vertices(0)}
        deformed = step("deformed")
        assert not (deformed["distance"] == posed["distance"]).all()
        g.bind_morphs(0, MORPHS)
        g.morph(weights={0: [0.7]})
        state["meshes"] = {"m1": g.mesh_vertices(0)}
        morphed = step("morphed")
        assert not (morphed["distance"] == deformed["distance"]).all()
        state["materials"] = {"red": dict(diffuse=(0.1, 0.7, 0.2, 1))}
        state["instance_materials"] = {2: "mirror", 0: None}
        table = g.materials()
        table[cases.MATERIAL_INDEX["red"]]["diffuse"] = (0.1, 0.7, 0.2, 1)
        g.relight(materials=table, instance_materials={2: cases.MATERIAL_INDEX["mirror"], 0: scenes.NO_MATERIAL})
        relit = step("relit")
        assert (relit["distance"] == morphed["distance"]).all() and not (relit["material"] == morphed["material"]).all()
    finally:
        g.close()


def test_nearest_leaves_a_live_frame_alone(case):
    """A progressive frame stopped after its first pass: the queries answer as without it, and the frame still finishes as process_job."""
    g, points, want = case["g"], case["points"], case["want"]
    opt = scenes.options(cases.FRAME_W, cases.FRAME_H, 4, 8)
    grid = ((-1.0, -1.0, 0.0), (0.25, 0.25, 0.25), (9, 9, 8))
    before = g.distance_grid(*grid)
    whole = g.process_job(cases.CAMERA, opt, base_seed=11)
    frame = binding.Frame(g, cases.CAMERA, opt, base_seed=11)
    try:
        frame.set_progressive(2, 1)
        _, _, info = frame.render()
        assert info["cancelled"]
        ref.assert_records_equal(g.nearest(points), want, "points beside a live frame")
        during = g.distance_grid(*grid)
        assert during[0].tobytes() == before[0].tobytes() and during[1].tobytes() == before[1].tobytes()
        frame.set_progressive(0)
        image, _, info = frame.render()
        assert info["status"] == binding.PT_OK
        assert_bits_equal(image, whole, "the frame after the queries")
    finally:
        frame.close()


def test_refusals(case):
    """PT_ERR_INVALID, before any device work: the arrays are never touched (the counts name far more than they hold)."""
    g = case["g"]
    lib, h, p = binding.load(), g._h, binding._ptr
    pts, recs, dist, obj = np.zeros((2, 4), F), np.full(2, 7, np.int32).repeat(16).view(binding.Nearest), np.full(8, 7.0, F), np.full(8, 7, np.int32)
    grid = binding.distance_grid((0, 0, 0), (1, 1, 1), (2, 2, 2))
    inf, n2, huge = C.c_float(np.inf), C.c_size_t(2), C.c_size_t(0x80000000)
    calls = [lambda: lib.pt_nearest_points(h, None, n2, p(recs)), lambda: lib.pt_nearest_points(h, p(pts), n2, None), lambda: lib.pt_nearest_points(h, p(pts), huge, p(recs)),
             lambda: lib.pt_nearest_points_device(h, None, n2, p(recs), None), lambda: lib.pt_nearest_points_device(h, p(pts), n2, None, None),
             lambda: lib.pt_nearest_points_device(h, p(pts), huge, p(recs), None),
             lambda: lib.pt_distance_grid_fill(h, None, inf, p(dist), p(obj)), lambda: lib.pt_distance_grid_fill(h, p(grid), inf, None, p(obj)),
             lambda: lib.pt_distance_grid_fill_device(h, None, inf, p(dist), p(obj), None), lambda: lib.pt_distance_grid_fill_device(h, p(grid), inf, None, p(obj), None)]
    for count in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (65536, 32768, 1), (2048, 1024, 1024), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        bad = binding.distance_grid((0, 0, 0), (1, 1, 1), count)
        calls += [lambda bad=bad: lib.pt_distance_grid_fill(h, p(bad), inf, p(dist), p(obj)), lambda bad=bad: lib.pt_distance_grid_fill_device(h, p(bad), inf, p(dist), p(obj), None)]
    for k, call in enumerate(calls):
        assert call() == 1, k  # PT_ERR_INVALID
    assert (recs.view(np.int32) == 7).all() and (dist == 7.0).all() and (obj == 7).all()
    assert lib.pt_nearest_points(h, None, C.c_size_t(0), None) == 0 and lib.pt_nearest_points_device(h, None, C.c_size_t(0), None, None) == 0  # n == 0: PT_OK, no launch
    # the largest grids that pass the count test are not tried: 0x7fffffff cells are 8 GB of distances


DEVICE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding
from tests import query_cases as cases
scene, _, _ = cases.build(sys.argv[2] == "L")
g = binding.Scene(scene, device=0)
rng = np.random.default_rng(5)
first, count = g.instance_ranges()
corners = g.triangles(int(first[0]), int(count.sum()))[0].reshape(-1, 3)
points = np.concatenate([rng.uniform(-1.5, 1.5, (700, 3)) + np.array([0.0, 0.0, 0.9]), corners[rng.choice(len(corners), 300, replace=False)]]).astype(np.float32)
q = np.concatenate([points, np.where(np.arange(1000) % 2 == 0, np.float32(np.inf), np.float32(0.3))[:, None]], axis=1).astype(np.float32)
grid = binding.distance_grid((-1.0, -1.0, 0.0), (0.25, 0.25, 0.25), (9, 9, 8))
stream = torch.cuda.current_stream(0).cuda_stream
def same(name, got, want):
    ok = got.tobytes() == want.tobytes()
    print("%s: %s" % (name, "bit-identical" if ok else "DIFFERENT"))
    return ok
ok = True
want = g.nearest(q[:, :3], q[:, 3])
assert 0.2 < (want["object"] >= 0).mean() < 1.0
distance, obj = g.distance_grid(grid, None, None, 0.6)
for s in (stream, 0):
    d_q = torch.from_numpy(q).to("cuda:0")
    d_out = torch.full((len(q), 16), -7, dtype=torch.int32, device="cuda:0")
    g.nearest_device(d_q.data_ptr(), len(q), d_out.data_ptr(), s)
    ok &= same("points", d_out.cpu().numpy().view(binding.Nearest).ravel(), want)
    d_distance = torch.full((8, 9, 9), -7.0, dtype=torch.float32, device="cuda:0")
    d_object = torch.full((8, 9, 9), -7, dtype=torch.int32, device="cuda:0")
    g.distance_grid_device(grid, d_distance.data_ptr(), d_object.data_ptr(), 0.6, s)
    ok &= same("grid distance", d_distance.cpu().numpy(), distance)
    ok &= same("grid object", d_object.cpu().numpy(), obj)
    d_alone = torch.full((8, 9, 9), -7.0, dtype=torch.float32, device="cuda:0")
    g.distance_grid_device(grid, d_alone.data_ptr(), 0, 0.6, s)
    ok &= same("grid distance alone", d_alone.cpu().numpy(), distance)
g.close()
sys.exit(0 if ok else 1)
"""


@pytest.mark.parametrize("name", ["S", "L"])
def test_device_forms_give_the_same_bytes(name):
    """Every _device entry point, on torch's stream and on the null stream, against its host form.  In a fresh interpreter in which torch
    opens the device first, as tests/test_gpu_query.py's."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT, name], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("bit-identical") == 8, r.stdout
