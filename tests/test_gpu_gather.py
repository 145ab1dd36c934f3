"""Light gathered at points on the GPU (include/pt_gather.h).  All comparisons are exact: pt_gather_points against the
yardstick tests/gather_ref.py on the oracle, values and counts bit for bit, for the three kinds on scenes S (tree in LDS), L (device-built,
records in HBM, walks that outgrow the stack's LDS window) and G (glass, both emitter kinds, point lights, a one-way mirror) of
tests/gather_cases.py; every chunk size gives the same bits; the device form equals the host form; a frame's gather and an instance's
bake equal the gather at the same points; after a pose and a relight the scene answers as a fresh one; and a live frame is left alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cpupathtrace_amd import binding, scenes
from tests import gather_cases as cases, gather_ref as ref, pose_probe, query_cases
from tests import motion_shapes_cases as msc
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EPSILON = cases.OPTIONS["epsilon"]
KINDS = [binding.GATHER_OCCLUSION, binding.GATHER_DIRECT, binding.GATHER_PATHS]
KIND_NAMES = {binding.GATHER_OCCLUSION: "occlusion", binding.GATHER_DIRECT: "direct", binding.GATHER_PATHS: "paths"}
_cache = {}


@pytest.fixture(scope="module")
def assembler(tmp_path_factory):
    return pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("gather_pose") / "libpose_probe.so")))


@pytest.fixture(scope="module", params=["S", "L", "G"])
def case(request, oracle_lib, assembler):
    """A scene on the device and flattened for the oracle, and its points; the yardstick's records are computed once per (kind, samples)."""
    name = request.param
    if name not in _cache:
        scene, instances, shapes = cases.build(name)
        flat = query_cases.flatten(scene, instances, shapes, assembler)
        handle = oracle_lib.scene_create(flat["scene"])
        pos, nrm = cases.points(handle, flat, name)
        _cache[name] = dict(name=name, scene=scene, flat=flat, handle=handle, pos=pos, nrm=nrm, g=binding.Scene(scene), want={})
    return _cache[name]


def _distance(kind):
    return cases.DISTANCE if kind == binding.GATHER_OCCLUSION else np.inf


def _want(case, kind, samples):
    """The yardstick's records of all the case's points (a point's record does not depend on how many follow it)."""
    key = (kind, samples)
    if key not in case["want"]:
        case["want"][key] = ref.gather(case["handle"], case["flat"], kind, case["pos"], case["nrm"], samples, EPSILON, _distance(kind), cases.SEED)
    return case["want"][key]


@pytest.mark.parametrize("samples", cases.SAMPLES)
@pytest.mark.parametrize("kind", KINDS)
def test_points_against_the_yardstick(case, kind, samples):
    g = case["g"]
    want = _want(case, kind, samples)
    for n in cases.BATCHES:
        got = g.gather(case["pos"][:n], case["nrm"][:n], kind, samples, EPSILON, _distance(kind), cases.SEED)
        ref.assert_records_equal(got, want[:n], "%s, %s, %d points x %d samples" % (case["name"], KIND_NAMES[kind], n, samples))
    assert (want["samples"] == samples).all() and (want["value"][:, 3] == 1).all()
    if kind == binding.GATHER_OCCLUSION:
        assert (want["occluded"] <= samples).all()
    else:
        assert (want["occluded"] == 0).all()
    print("%s %s x %d: mean value %s, occluded %d of %d" % (case["name"], KIND_NAMES[kind], samples, want["value"][:, :3].mean(axis=0), want["occluded"].sum(), samples * len(want)))


def test_occlusion_without_a_distance_and_an_empty_call(case):
    g = case["g"]
    want = ref.gather(case["handle"], case["flat"], binding.GATHER_OCCLUSION, case["pos"][:65], case["nrm"][:65], 2, EPSILON, np.inf, 5)
    ref.assert_records_equal(g.gather(case["pos"][:65], case["nrm"][:65], binding.GATHER_OCCLUSION, 2, EPSILON, base_seed=5), want, "distance +inf")
    assert len(g.gather(np.zeros((0, 3), F), np.zeros((0, 3), F), binding.GATHER_PATHS, 4, EPSILON)) == 0
    with pytest.raises(binding.PtError) as e:
        g.bake_instance(len(g.instance_ranges()[0]), binding.GATHER_DIRECT, 1, EPSILON)
    assert e.value.code == 1 and "out of range" in str(e.value)
    out = np.zeros(3, binding.GatherResult)
    gp = binding.gather_params(binding.GATHER_DIRECT, 1, EPSILON)
    assert binding.load().pt_gather_instance(g._h, C.c_uint32(1000), C.byref(gp), binding._ptr(out)) == 1 and b"out of range" in binding.load().pt_last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_chunks_change_no_bit(case, kind):
    """PT_GATHER_CHUNK is read per call and counts (point, sample) pairs: 17 holds exactly one point of 17 samples, 64 three, 1000 58."""
    g, n, samples = case["g"], 65, 17
    want = _want(case, kind, samples)[:n]
    whole = g.gather(case["pos"][:n], case["nrm"][:n], kind, samples, EPSILON, _distance(kind), cases.SEED)
    ref.assert_records_equal(whole, want, "the default chunk")
    before = os.environ.get("PT_GATHER_CHUNK")
    try:
        for chunk in (17, 64, 1000):
            os.environ["PT_GATHER_CHUNK"] = str(chunk)
            got = g.gather(case["pos"][:n], case["nrm"][:n], kind, samples, EPSILON, _distance(kind), cases.SEED)
            ref.assert_records_equal(got, whole, "%s, %s, chunks of %d pairs" % (case["name"], KIND_NAMES[kind], chunk))
        os.environ["PT_GATHER_CHUNK"] = "1"  # less than a point: one point per launch
        got = g.gather(case["pos"][:9], case["nrm"][:9], kind, samples, EPSILON, _distance(kind), cases.SEED)
        ref.assert_records_equal(got, whole[:9], "one point per launch")
    finally:
        if before is None:
            del os.environ["PT_GATHER_CHUNK"]
        else:
            os.environ["PT_GATHER_CHUNK"] = before


def _flipped(frame):
    """id_map's positions and normals with the normals turned against the rays, on the host: (hit mask, positions, normals)."""
    frame = frame.ravel()
    hit = frame["object"] >= 0
    pixels = query_cases.frame_pixels(cases.FRAME_W, cases.FRAME_H)
    return hit, frame["position"][hit], frame["normal"][hit], pixels[hit]


@pytest.mark.parametrize("kind", KINDS)
def test_a_frame_is_the_gather_at_its_first_hits(case, oracle_lib, kind):
    g, samples = case["g"], 2
    frame = g.id_map(cases.CAMERA, cases.OPTIONS)
    hit, pos, nrm, pixels = _flipped(frame)
    d = query_cases.pixel_rays(oracle_lib, cases.CAMERA, cases.FRAME_W, cases.FRAME_H, pixels)[:, 3:]
    away = ref._dot(nrm.astype(F), d.astype(F)) > 0
    nrm = np.where(away[:, None], -nrm, nrm).astype(F)
    assert 0.3 <= hit.mean() and (case["name"] == "G" or hit.mean() < 1.0)  # (G is a closed room: every pixel hits)
    got = g.gather_frame(cases.CAMERA, cases.OPTIONS, kind, samples, EPSILON, _distance(kind), cases.SEED)
    assert got.shape == (cases.FRAME_H, cases.FRAME_W)
    got = got.ravel()
    assert got[~hit].tobytes() == np.zeros((~hit).sum(), binding.GatherResult).tobytes()
    # point i of a frame is pixel i: gather the hits at their pixels' indices, with anything in between
    all_pos, all_nrm = np.zeros((len(hit), 3), F), np.tile(np.array([0, 1, 0], F), (len(hit), 1))
    all_pos[hit], all_nrm[hit] = pos, nrm
    want = g.gather(all_pos, all_nrm, kind, samples, EPSILON, _distance(kind), cases.SEED)
    ref.assert_records_equal(got[hit], want[hit], "frame of %s, %s" % (case["name"], KIND_NAMES[kind]))
    # an aperture is not sampled
    lens = dict(cases.CAMERA, aperture_width=0.1, aperture_height=0.1, aperture_kind=scenes.APERTURE_CIRCULAR)
    assert g.gather_frame(lens, cases.OPTIONS, kind, samples, EPSILON, _distance(kind), cases.SEED).tobytes() == got.tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_a_bake_is_the_gather_at_the_corners(case, kind):
    """Every instance: S and L have the smooth patch twice and the flat mesh that lost its degenerate faces, L the large grid as well."""
    g, samples = case["g"], 2
    first, count = g.instance_ranges()
    assert len(first) >= 3
    for i in range(len(first)):
        pos, nrm, _, _ = g.triangles(int(first[i]), int(count[i]))
        got = g.bake_instance(i, kind, samples, EPSILON, _distance(kind), cases.SEED)
        assert got.shape == (int(count[i]), 3)
        want = g.gather(pos.reshape(-1, 3), nrm.reshape(-1, 3), kind, samples, EPSILON, _distance(kind), cases.SEED)
        ref.assert_records_equal(got.ravel(), want, "instance %d of %s, %s" % (i, case["name"], KIND_NAMES[kind]))
    if case["name"] != "G":
        assert count[:3].tolist() == [72, 72, 35]  # (the third kept 35 of its 40 faces)


def _answers(g, pos, nrm):
    out = []
    for kind in KINDS:
        out.append(g.gather(pos, nrm, kind, 2, EPSILON, _distance(kind), cases.SEED))
        out.append(g.gather_frame(cases.CAMERA, cases.OPTIONS, kind, 1, EPSILON, _distance(kind), cases.SEED).ravel())
        out.append(g.bake_instance(0, kind, 1, EPSILON, _distance(kind), cases.SEED).ravel())
    return out


LIGHTS = (np.array([[0.5, 0.8, -0.5]], F), np.array([[0.1, 0.2, 0.9, 1.0]], F))


def _fresh(state, lights=None):
    """Scene S created afresh in `state`; query_cases.build places one fixed point light, so other lights are put into the description."""
    scene, _, _ = query_cases.build(False, **state)
    if lights is not None:
        scene["light_pos"], scene["light_spectrum"] = lights
    return binding.Scene(scene)


def test_gathers_follow_the_scene_in_place(oracle_lib, assembler):
    """Scene S through a pose and a relight: after each, every gather equals the same gather on a scene created afresh in the new state."""
    scene, instances, shapes = query_cases.build(False)
    flat = query_cases.flatten(scene, instances, shapes, assembler)
    handle = oracle_lib.scene_create(flat["scene"])
    pos, nrm = cases.points(handle, flat, "S")
    handle.close()
    pos, nrm = pos[:65], nrm[:65]
    g = binding.Scene(scene)
    state = dict(matrices=[m for _, m, _, _, _ in instances], materials={})
    try:
        def step(what, lights=None):
            fresh = _fresh(state, lights)
            try:
                want, got = _answers(fresh, pos, nrm), _answers(g, pos, nrm)
                for k, (a, b) in enumerate(zip(got, want)):
                    ref.assert_records_equal(a, b, "%s: answer %d" % (what, k))
                return want
            finally:
                fresh.close()

        before = step("as created")
        state["matrices"][0] = msc.place(-0.4, -0.3, 0.55, 0.75, degrees=12.0)
        state["matrices"][2] = msc.place(0.05, 0.0, 1.0, 1.1, degrees=5.0)
        g.pose([state["matrices"][0], state["matrices"][2]], instances=[0, 2])
        posed = step("posed")
        assert any(a.tobytes() != b.tobytes() for a, b in zip(posed, before))
        state["materials"] = {"glow": dict(emission=(0.2, 1.0, 0.3, 3.0))}
        table = g.materials()
        table[query_cases.MATERIAL_INDEX["glow"]]["emission"] = (0.2, 1.0, 0.3, 3.0)
        g.relight(materials=table, point_lights=LIGHTS)
        relit = step("relit", LIGHTS)
        assert relit[0].tobytes() == posed[0].tobytes() and relit[3].tobytes() != posed[3].tobytes()  # occlusion stays, the direct light changed
    finally:
        g.close()


def test_gathers_leave_a_live_frame_alone(case):
    """A progressive frame stopped after its first pass, gathers of every kind in between: the frame finishes as process_job renders it."""
    g = case["g"]
    opt = scenes.options(cases.FRAME_W, cases.FRAME_H, 4, 8)
    pos, nrm = case["pos"][:65], case["nrm"][:65]
    before = _answers(g, pos, nrm)
    whole = g.process_job(cases.CAMERA, opt, base_seed=11)
    frame = binding.Frame(g, cases.CAMERA, opt, base_seed=11)
    try:
        frame.set_progressive(2, 1)
        _, _, info = frame.render()
        assert info["cancelled"]
        during = _answers(g, pos, nrm)
        for k, (a, b) in enumerate(zip(during, before)):
            ref.assert_records_equal(a, b, "beside a live frame: answer %d" % k)
        frame.set_progressive(0)
        image, _, info = frame.render()
        assert info["status"] == binding.PT_OK
        assert_bits_equal(image, whole, "the frame after the gathers")
    finally:
        frame.close()


DEVICE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding
from tests import gather_cases as cases
scene, _, _ = cases.build(sys.argv[2])
g = binding.Scene(scene, device=0)
rng = np.random.default_rng(4)
frame = g.id_map(cases.CAMERA, cases.OPTIONS).ravel()
hit = frame[frame["object"] >= 0][:130]
pts = np.ascontiguousarray(np.concatenate([hit["position"], hit["normal"]], axis=1), np.float32)
stream = torch.cuda.current_stream(0).cuda_stream
ok = True
for s in (stream, 0):
    for kind in (0, 1, 2):
        distance = cases.DISTANCE if kind == 0 else np.inf
        d_pts = torch.from_numpy(pts).to("cuda:0")
        d_out = torch.full((len(pts), 8), -7, dtype=torch.int32, device="cuda:0")
        g.gather_device(d_pts.data_ptr(), len(pts), d_out.data_ptr(), kind, 3, 1e-3, distance, cases.SEED, s)
        same = d_out.cpu().numpy().view(binding.GatherResult).ravel().tobytes() == g.gather(pts[:, :3], pts[:, 3:], kind, 3, 1e-3, distance, cases.SEED).tobytes()
        d_frame = torch.full((len(frame), 8), -7, dtype=torch.int32, device="cuda:0")
        g.gather_frame_device(cases.CAMERA, cases.OPTIONS, d_frame.data_ptr(), kind, 2, 1e-3, distance, cases.SEED, s)
        same_frame = d_frame.cpu().numpy().view(binding.GatherResult).ravel().tobytes() == g.gather_frame(cases.CAMERA, cases.OPTIONS, kind, 2, 1e-3, distance, cases.SEED).tobytes()
        print("kind %d: points %s, frame %s" % (kind, "bit-identical" if same else "DIFFERENT", "bit-identical" if same_frame else "DIFFERENT"))
        ok &= same and same_frame
g.close()
sys.exit(0 if ok else 1)
"""


@pytest.mark.parametrize("name", ["S", "L"])
def test_device_forms_give_the_same_bytes(name):
    """pt_gather_points_device and pt_gather_frame_device on torch's stream and on the null stream against their host forms, in a fresh
    interpreter in which torch opens the device first (tests/test_gpu_query.py's arrangement)."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT, name], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("bit-identical") == 12, r.stdout
