"""Scene queries on the GPU (include/pt_query.h): pt_query_rays has pt_intersect_batch's t and object bit for bit and the
whole record of tests/query_ref.py bit for bit; pt_occluded_rays is 0 <= t < t_max of pt_intersect_batch's t at every threshold;
pt_query_pixels and pt_query_frame are pt_query_rays on the oracle's camera rays through the pixel centres; instance and face follow
pt_scene_instance_ranges and the face table; after a pose, a deformation, a morph and a relight every query is what a freshly created
scene of the new state answers; and queries leave a live frame as it was.  Scenes S (tree in LDS) and L (device-built, records in HBM,
walks that outgrow the stack's LDS window) of tests/query_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cpupathtrace_amd import binding, scenes
from tests import motion_shapes_cases as msc
from tests import pose_probe, query_cases as cases, query_ref
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
_cache = {}


@pytest.fixture(scope="module")
def assembler(tmp_path_factory):
    return pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("query_pose") / "libpose_probe.so")))


@pytest.fixture(scope="module", params=["S", "L"])
def case(request, oracle_lib, assembler):
    """A scene on the device and flattened for the oracle, its rays, and the restated records of all of them (computed once)."""
    name = request.param
    if name not in _cache:
        scene, instances, shapes = cases.build(name == "L")
        flat = cases.flatten(scene, instances, shapes, assembler)
        handle = oracle_lib.scene_create(flat["scene"])
        rays = cases.rays(flat)
        _cache[name] = dict(name=name, flat=flat, handle=handle, rays=rays, want=query_ref.records(handle, flat, rays), g=binding.Scene(scene))
    return _cache[name]


def test_rays_are_intersect_batch_and_the_restatement(case):
    g, rays = case["g"], case["rays"]
    info = g.info()
    if case["name"] == "L":
        assert g.n_objects >= 1024 and info["depth"] > 10, (g.n_objects, info)
    else:
        assert g.n_objects < 1024
    for n in cases.BATCHES:
        got = g.query(rays[:n])
        t, obj = g.get_intersection(rays[:n])
        assert_bits_equal(got["t"], t, "%s, %d rays: t" % (case["name"], n))
        assert (got["object"] == obj).all()
        query_ref.assert_records_equal(got, case["want"][:n], "%s, %d rays" % (case["name"], n))
    assert len(g.query(np.zeros((0, 6), F))) == 0
    hit = case["want"]["object"] >= 0
    print("%s: %d of %d rays hit; %d without a face, %d on instances" % (case["name"], hit.sum(), len(hit), (case["want"]["face"][hit] == query_ref.NO_FACE).sum(),
                                                                       (case["want"]["instance"] >= 0).sum()))


def test_occlusion_is_the_closest_hit_below_the_threshold(case):
    g, rays = case["g"], case["rays"]
    t, _ = g.get_intersection(rays)
    idx, t_max = cases.thresholds(t)
    with np.errstate(invalid="ignore"):
        want = (t[idx] >= 0) & (t[idx] < t_max)
    assert 0.3 <= want.mean() <= 0.7
    got = g.occluded(rays[idx], t_max)
    assert (got == want).all(), (np.nonzero(got != want)[0][:5], t[idx][got != want][:5], t_max[got != want][:5])
    # rays that hit nothing are never occluded, whatever the threshold; and every batch size gives the whole batch's answers
    assert not g.occluded(rays[t < 0], np.inf).any()
    for n in cases.BATCHES:
        assert (g.occluded(rays[idx[:n]], t_max[:n]) == want[:n]).all(), n
    assert len(g.occluded(np.zeros((0, 6), F), np.zeros(0, F))) == 0


def test_pixels_and_frames_are_the_rays_through_pixel_centres(case, oracle_lib):
    g = case["g"]
    pixels = cases.frame_pixels(cases.FRAME_W, cases.FRAME_H)
    want = g.query(cases.pixel_rays(oracle_lib, cases.CAMERA, cases.FRAME_W, cases.FRAME_H, pixels))
    assert (want["object"] >= 0).mean() >= 0.3
    frame = g.id_map(cases.CAMERA, cases.OPTIONS)
    assert frame.shape == (cases.FRAME_H, cases.FRAME_W)
    query_ref.assert_records_equal(frame.ravel(), want, "frame of %s" % case["name"])
    query_ref.assert_records_equal(g.pick(cases.CAMERA, cases.OPTIONS, pixels), want, "all pixels of %s" % case["name"])
    some = np.random.default_rng(3).permutation(len(pixels))[:65]
    query_ref.assert_records_equal(g.pick(cases.CAMERA, cases.OPTIONS, pixels[some]), want[some], "65 pixels of %s" % case["name"])
    # an aperture is not sampled: the rays are a pure function of camera and pixel
    lens = dict(cases.CAMERA, aperture_width=0.1, aperture_height=0.1, aperture_kind=scenes.APERTURE_CIRCULAR)
    query_ref.assert_records_equal(g.id_map(lens, cases.OPTIONS).ravel(), want, "with a lens")
    for outside in ([cases.FRAME_W, 0], [0, cases.FRAME_H], [-1, 3], [2, -1]):
        with pytest.raises(binding.PtError) as e:
            g.pick(cases.CAMERA, cases.OPTIONS, [[1, 1], outside])
        assert e.value.code == 1 and "outside the frame" in str(e.value)
    assert len(g.pick(cases.CAMERA, cases.OPTIONS, np.zeros((0, 2), np.int32))) == 0


def test_the_frame_agrees_with_the_feature_pass_on_a_wall():
    """A camera in front of one large flat triangle: the four sub-pixel rays of pt_render_features cannot differ from the centre ray in
    what they hit, so coverage 1 everywhere means object 0 everywhere, and looking away coverage 0 means a miss everywhere."""
    sb = scenes.SceneBuilder()
    sb.triangles([[[-50.0, -50.0, 2.0], [0.0, 80.0, 2.0], [50.0, -50.0, 2.0]]])
    g = binding.Scene(sb.build())
    try:
        for cam, hits in ((cases.CAMERA, True), (dict(cases.CAMERA, look_at=(0.0, 0.0, -3.0)), False)):
            features, frame = g.render_features(cam, cases.OPTIONS), g.id_map(cam, cases.OPTIONS)
            assert (features[..., 0, 3] == (1.0 if hits else 0.0)).all()
            assert (frame["object"] == (0 if hits else -1)).all() and ((frame["t"] >= 0) == hits).all()
            assert (frame["instance"] == -1).all() and (frame["face"] == query_ref.NO_FACE).all()
    finally:
        g.close()


def test_instances_and_faces_follow_the_ranges_and_the_face_table(case):
    g, rays, flat = case["g"], case["rays"], case["flat"]
    first, count = g.instance_ranges()
    assert first.tolist() == flat["first"].tolist() and count.tolist() == flat["count"].tolist()
    got = g.query(rays)
    obj = got["object"].astype(np.int64)
    want_instance = np.full(len(obj), -1)
    for i in range(len(first)):
        want_instance[(obj >= int(first[i])) & (obj < int(first[i]) + int(count[i]))] = i
    assert (got["instance"] == want_instance).all() and len(np.unique(want_instance)) == len(first) + 1
    m1, m2 = (got["instance"] == 0) | (got["instance"] == 1), got["instance"] == 2
    assert m1.any() and (got["face"][m1] == (obj - first[got["instance"]])[m1]).all()          # rule (a)
    assert m2.any() and (got["face"][m2] == query_ref.NO_FACE).all()                            # no table yet
    assert (got["face"][got["instance"] < 0] == query_ref.NO_FACE).all()
    matrices = g.pose_transforms()
    g.mark_motion()
    try:
        query_ref.assert_records_equal(g.query(rays), got, "a mark alone")
        g.pose(matrices)  # (the same pose: the rebuild makes the table)
        table = g.triangle_faces()
        marked = g.query(rays)
        local = table[obj - flat["n_desc"]].astype(np.int64) - np.asarray(flat["face_first"])[got["instance"]]
        assert (marked["face"][m2] == local[m2]).all() and (marked["face"][m2] < 40).all()     # rule (b)
        assert (marked["face"][m1] == local[m1]).all() and (marked["face"][m1] == got["face"][m1]).all()  # both rules, one answer
        assert (marked["face"][m1 | m2] == flat["local_face"][obj[m1 | m2] - flat["n_desc"]]).all()
        query_ref.assert_records_equal(marked, query_ref.records(case["handle"], flat, rays, with_table=True), "with the table")
    finally:
        g.unmark_motion()
    query_ref.assert_records_equal(g.query(rays), got, "after the mark is gone")


MORPHS = [(None, np.stack([np.zeros(49, F), 0.05 * msc.patch()[0][:, 0], 0.12 * msc.patch()[0][:, 1]], axis=1).astype(F))]


def _answers(g, rays, idx, t_max):
    return g.query(rays), g.occluded(rays[idx], t_max), g.id_map(cases.CAMERA, cases.OPTIONS)


def test_queries_follow_the_scene_in_place():
    """Scene S through a pose, a deformation, a morph and a relight: after each, every query equals the same query on a scene created
    afresh in the new state (the rays keep hitting: at least 40 % of them every time)."""
    scene, instances, _ = cases.build(False)
    g = binding.Scene(scene)
    state = dict(matrices=[m for _, m, _, _, _ in instances], meshes={}, materials={}, instance_materials={})
    rays = cases.rays(_device_flat(g, scene))
    try:
        def step(what):
            fresh_scene, _, _ = cases.build(False, **state)
            fresh = binding.Scene(fresh_scene)
            try:
                t, _ = fresh.get_intersection(rays)
                assert (t >= 0).mean() >= 0.4, (what, (t >= 0).mean())
                idx, t_max = cases.thresholds(t)
                want, got = _answers(fresh, rays, idx, t_max), _answers(g, rays, idx, t_max)
                query_ref.assert_records_equal(got[0], want[0], what + ": rays")
                assert (got[1] == want[1]).all(), what
                query_ref.assert_records_equal(got[2], want[2], what + ": frame")
                return want[0]
            finally:
                fresh.close()

        before = step("as created")
        state["matrices"][0] = msc.place(-0.4, -0.3, 0.55, 0.75, degrees=12.0)
        state["matrices"][2] = msc.place(0.05, 0.0, 1.0, 1.1, degrees=5.0)
        g.pose([state["matrices"][0], state["matrices"][2]], instances=[0, 2])
        posed = step("posed")
        assert not (posed["t"] == before["t"]).all()
        g.deform(vertices={0: msc.patch_bent(0.15)})
        state["meshes"] = {"m1": g.mesh_vertices(0)}
        deformed = step("deformed")
        assert not (deformed["t"] == posed["t"]).all()
        g.bind_morphs(0, MORPHS)
        g.morph(weights={0: [0.7]})
        state["meshes"] = {"m1": g.mesh_vertices(0)}
        morphed = step("morphed")
        assert not (morphed["t"] == deformed["t"]).all()
        state["materials"] = {"red": dict(diffuse=(0.1, 0.7, 0.2, 1))}
        state["instance_materials"] = {2: "mirror", 0: None}
        table = g.materials()
        table[cases.MATERIAL_INDEX["red"]]["diffuse"] = (0.1, 0.7, 0.2, 1)
        g.relight(materials=table, instance_materials={2: cases.MATERIAL_INDEX["mirror"], 0: scenes.NO_MATERIAL})
        relit = step("relit")
        assert (relit["t"] == morphed["t"]).all() and not (relit["material"] == morphed["material"]).all()
    finally:
        g.close()


def _device_flat(g, scene):
    """What cases.rays reads of a flattened scene, from the device's own triangles."""
    first, count = g.instance_ranges()
    pos, _, _, _ = g.triangles(int(first[0]), int(count.sum()))
    flat = dict(tri_pos=np.concatenate([np.asarray(scene["tri_pos"], F).reshape(-1, 9), pos]), sph=scene["sph"], obj_kind=scene["obj_kind"])
    return dict(scene=flat, n_desc=int(first[0]), count=count)


def test_queries_leave_a_live_frame_alone(case):
    """A progressive frame stopped after its first pass: the queries answer as without it, and the frame still finishes as process_job."""
    g, rays = case["g"], case["rays"]
    opt = scenes.options(cases.FRAME_W, cases.FRAME_H, 4, 8)
    t, _ = g.get_intersection(rays)
    idx, t_max = cases.thresholds(t)
    before = _answers(g, rays, idx, t_max)
    whole = g.process_job(cases.CAMERA, opt, base_seed=11)
    frame = binding.Frame(g, cases.CAMERA, opt, base_seed=11)
    try:
        frame.set_progressive(2, 1)
        _, _, info = frame.render()
        assert info["cancelled"]
        during = _answers(g, rays, idx, t_max)
        query_ref.assert_records_equal(during[0], before[0], "rays beside a live frame")
        assert (during[1] == before[1]).all()
        query_ref.assert_records_equal(during[2], before[2], "frame beside a live frame")
        frame.set_progressive(0)
        image, _, info = frame.render()
        assert info["status"] == binding.PT_OK
        assert_bits_equal(image, whole, "the frame after the queries")
    finally:
        frame.close()


DEVICE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding
from tests import query_cases as cases
scene, _, _ = cases.build(sys.argv[2] == "L")
g = binding.Scene(scene, device=0)
first, count = g.instance_ranges()
pos, _, _, _ = g.triangles(int(first[0]), int(count.sum()))
flat = dict(scene=dict(tri_pos=np.concatenate([np.asarray(scene["tri_pos"], np.float32).reshape(-1, 9), pos]), sph=scene["sph"], obj_kind=scene["obj_kind"]),
            n_desc=int(first[0]), count=count)
rays = cases.rays(flat)
t, _ = g.get_intersection(rays)
idx, t_max = cases.thresholds(t)
seg = np.concatenate([rays[idx], t_max[:, None]], axis=1).astype(np.float32)
pixels = cases.frame_pixels(cases.FRAME_W, cases.FRAME_H)
stream = torch.cuda.current_stream(0).cuda_stream
def same(name, got, want):
    ok = got.tobytes() == want.tobytes()
    print("%s: %s" % (name, "bit-identical" if ok else "DIFFERENT"))
    return ok
ok = True
for s in (stream, 0):
    d_rays, d_seg, d_xy = torch.from_numpy(rays).to("cuda:0"), torch.from_numpy(seg).to("cuda:0"), torch.from_numpy(pixels).to("cuda:0")
    d_hits = torch.full((len(rays), 16), -7, dtype=torch.int32, device="cuda:0")
    g.query_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), s)
    ok &= same("rays", d_hits.cpu().numpy().view(binding.Hit).ravel(), g.query(rays))
    d_flags = torch.full((len(seg),), 9, dtype=torch.uint8, device="cuda:0")
    g.occluded_device(d_seg.data_ptr(), len(seg), d_flags.data_ptr(), s)
    ok &= same("segments", d_flags.cpu().numpy(), g.occluded(rays[idx], t_max).astype(np.uint8))
    d_px = torch.full((len(pixels), 16), -7, dtype=torch.int32, device="cuda:0")
    g.pick_device(cases.CAMERA, cases.OPTIONS, d_xy.data_ptr(), len(pixels), d_px.data_ptr(), s)
    ok &= same("pixels", d_px.cpu().numpy().view(binding.Hit).ravel(), g.pick(cases.CAMERA, cases.OPTIONS, pixels))
    d_frame = torch.full((len(pixels), 16), -7, dtype=torch.int32, device="cuda:0")
    g.id_map_device(cases.CAMERA, cases.OPTIONS, d_frame.data_ptr(), s)
    ok &= same("frame", d_frame.cpu().numpy().view(binding.Hit).ravel(), g.id_map(cases.CAMERA, cases.OPTIONS).ravel())
g.close()
sys.exit(0 if ok else 1)
"""


@pytest.mark.parametrize("name", ["S", "L"])
def test_device_forms_give_the_same_bytes(name):
    """Every _device entry point, on torch's stream and on the null stream, against its host form.  In a fresh interpreter in which torch
    opens the device first, as tests/test_gpu_motion.py's."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT, name], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("bit-identical") == 8, r.stdout
