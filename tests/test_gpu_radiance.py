"""Radiance along free rays and captures on the GPU (include/pt_radiance.h).  Every comparison is exact: pt_radiance_rays
against the yardstick tests/radiance_ref.py on the oracle, values and counts bit for bit, on scenes S (tree in LDS), L (device-built,
records in HBM, walks that outgrow the stack's LDS window) and G (glass, both emitter kinds, point lights, a one-way mirror) with the rays
of tests/radiance_cases.py; every chunk size gives the same bits; the four capture models equal the yardstick's generators with and
without jitter; a capture without jitter is the rays call on its centre rays; the device forms equal the host forms; a live frame is left
alone; and in a furnace every pixel of every model is the emission."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cpupathtrace_amd import binding, scenes
from tests import light_probe_cases, pose_probe, query_cases, radiance_cases as cases, radiance_ref as ref
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EPSILON = cases.OPTIONS["epsilon"]
MOST = max(cases.SAMPLES)
CAPTURE_SAMPLES = [1, 65]


@pytest.fixture(scope="module")
def assembler(tmp_path_factory):
    return pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("radiance_pose") / "libpose_probe.so")))


@pytest.fixture(scope="module", params=["S", "L", "G"])
def case(request, oracle_lib, assembler):
    """A scene on the device and flattened for the oracle, its rays, and the yardstick's samples of all of them, computed once: sample s
    of ray i has its own engine, so the first k samples of the largest count are the samples of a call with k.  The scene is closed
    behind the module's last test of it, so that nothing of it stays on the device for the tests that follow."""
    name = request.param
    scene, instances, shapes = cases.build(name)
    flat = query_cases.flatten(scene, instances, shapes, assembler)
    handle = oracle_lib.scene_create(flat["scene"])
    rays = cases.rays(flat)
    L, missed, _ = ref.ray_samples(handle, flat, rays, MOST, EPSILON, cases.SEED)
    g = binding.Scene(scene)
    yield dict(name=name, scene=scene, flat=flat, handle=handle, rays=rays, samples=(L, missed), g=g, want={})
    g.close()
    handle.close()


def _want(case, samples):
    """The yardstick's records of all the case's rays at a sample count (a ray's record does not depend on how many follow it)."""
    if samples not in case["want"]:
        L, missed = case["samples"]
        case["want"][samples] = ref.records(L[:, :samples], missed[:, :samples])
    return case["want"][samples]


@pytest.mark.parametrize("samples", cases.SAMPLES)
def test_rays_against_the_yardstick(case, samples):
    g, want = case["g"], _want(case, samples)
    for n in cases.BATCHES:
        got = g.radiance(case["rays"][:n], samples, EPSILON, cases.SEED)
        ref.assert_records_equal(got, want[:n], "%s, %d rays x %d samples" % (case["name"], n, samples))
    assert (want["samples"] == samples).all() and (want["outside"] == 0).all() and ((want["missed"] == 0) | (want["missed"] == samples)).all()
    if samples == 1:
        # value is L_0: paths_from_rays's rgba, bit for bit
        got = g.radiance(case["rays"], 1, EPSILON, cases.SEED)
        L = case["samples"][0][:, 0]
        assert ((got["value"].view(np.uint32) == L.view(np.uint32)) | (np.isnan(got["value"]) & np.isnan(L))).all()
    print("%s x %d: mean value %s, rays that miss %d of %d" % (case["name"], samples, np.nanmean(want["value"], axis=0), (want["missed"] > 0).sum(), len(want)))


def test_an_empty_call(case):
    assert len(case["g"].radiance(np.zeros((0, 6), F), 4, EPSILON)) == 0


def test_chunks_change_no_bit(case):
    """PT_RADIANCE_CHUNK is read per call and counts (ray, sample) pairs: with 17 samples a chunk of 17 holds exactly one ray, 64 three,
    1000 58; 1 is less than a ray: one ray per launch.  With 65 samples -- more than one strided round per ray -- 130 pairs hold two rays,
    200 three (and 5 spare), everything below 65 one."""
    g, n = case["g"], 65
    before = os.environ.get("PT_RADIANCE_CHUNK")
    try:
        for samples in (17, 65):
            os.environ.pop("PT_RADIANCE_CHUNK", None)
            whole = g.radiance(case["rays"][:n], samples, EPSILON, cases.SEED)
            ref.assert_records_equal(whole, _want(case, samples)[:n], "the default chunk")
            for chunk in cases.CHUNKS:
                os.environ["PT_RADIANCE_CHUNK"] = str(chunk)
                got = g.radiance(case["rays"][:n], samples, EPSILON, cases.SEED)
                ref.assert_records_equal(got, whole, "%s, %d samples, chunks of %d pairs" % (case["name"], samples, chunk))
        os.environ["PT_RADIANCE_CHUNK"] = "64"  # a ray that alone has more pairs gets a launch of its own
        got = g.radiance(case["rays"][:5], 130, EPSILON, cases.SEED)
        ref.assert_records_equal(got, _want(case, 130)[:5], "rays larger than a chunk")
        # a capture is cut into whole pixels in the same way
        desc = cases.desc(binding.CAPTURE_CUBE, 18, 3, cases.origins(case["name"])[0], True)
        os.environ.pop("PT_RADIANCE_CHUNK", None)
        whole = g.capture(desc, 17, EPSILON, cases.SEED)
        for chunk in (1, 64, 200):
            os.environ["PT_RADIANCE_CHUNK"] = str(chunk)
            ref.assert_records_equal(g.capture(desc, 17, EPSILON, cases.SEED), whole, "%s, a capture in chunks of %d pairs" % (case["name"], chunk))
    finally:
        if before is None:
            os.environ.pop("PT_RADIANCE_CHUNK", None)
        else:
            os.environ["PT_RADIANCE_CHUNK"] = before


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("label,model,width,height,kw", cases.SMALL, ids=[c[0] for c in cases.SMALL])
def test_captures_against_the_yardstick(case, label, model, width, height, kw, jitter):
    g = case["g"]
    for view in cases.origins(case["name"]):
        desc = cases.desc(model, width, height, view, jitter, **kw)
        L, missed, outside, _ = ref.capture_samples(case["handle"], case["flat"], desc, max(CAPTURE_SAMPLES), EPSILON, cases.SEED)
        for samples in CAPTURE_SAMPLES:
            want = ref.records(L[:, :samples], missed[:, :samples], outside[:, :samples]).reshape(height, width)
            got = g.capture(desc, samples, EPSILON, cases.SEED)
            ref.assert_records_equal(got, want, "%s of %s from %s, jitter %d, %d samples" % (label, case["name"], view[0], jitter, samples))
        print("%s of %s from %s, jitter %d: missed %d, outside %d of %d" % (label, case["name"], view[0], jitter, want["missed"].sum(), want["outside"].sum(), want["samples"].sum()))
        if model == binding.CAPTURE_FISHEYE:
            # checked on the yardstick first (here at 65 samples): without jitter the corner pixels have no ray at all; jitter softens the
            # circle's edge
            corners, partly = want[[0, 0, 4, 4], [0, 4, 0, 4]], (want["outside"] > 0) & (want["outside"] < samples)
            if jitter:
                assert partly.sum() >= 8 and partly[[0, 0, 4, 4], [0, 4, 0, 4]].all()
            else:
                assert (corners["outside"] == samples).all() and (corners["value"] == 0).all() and (corners["missed"] == 0).all() and not partly.any()
                assert (got[[0, 0, 4, 4], [0, 4, 0, 4]]["value"] == 0).all() and (got[[0, 0, 4, 4], [0, 4, 0, 4]]["outside"] == samples).all()
        if model == binding.CAPTURE_ORTHO and view is cases.origins(case["name"])[0]:
            assert (want["missed"] == samples).any() and (want["missed"] < samples).any()  # the window is wider than the scene: some pixels miss


@pytest.mark.parametrize("label,model,width,height,kw", cases.LARGE, ids=[c[0] for c in cases.LARGE])
def test_a_capture_without_jitter_is_the_rays_call(case, label, model, width, height, kw):
    """Device against device: pixel i and ray i share their engines, and without jitter nothing is drawn before the loop."""
    g, samples = case["g"], 3
    desc = cases.desc(model, width, height, cases.origins(case["name"])[-1], False, **kw)
    rays, outside = ref.centre_rays(desc)
    rays[outside, 3:] = (0.0, 0.0, 1.0)  # (a pixel without a ray: any ray will do, its answer is not compared)
    got = g.capture(desc, samples, EPSILON, cases.SEED).ravel()
    want = g.radiance(rays, samples, EPSILON, cases.SEED)
    assert ((got["outside"] == samples) == outside).all() and ((got["outside"] == 0) == ~outside).all()
    assert outside.any() == (model == binding.CAPTURE_FISHEYE) and (~outside).sum() >= 0.7 * len(rays)
    ref.assert_records_equal(got[~outside], want[~outside], "%s of %s" % (label, case["name"]))
    assert (got["value"][outside] == 0).all() and (got["missed"][outside] == 0).all() and (got["samples"] == samples).all()


def test_radiance_calls_leave_a_live_frame_alone(case):
    """A progressive frame stopped after its first pass, calls of both kinds in between: the frame finishes as process_job renders it,
    and the calls answer as without it."""
    g = case["g"]
    opt = scenes.options(cases.FRAME_W, cases.FRAME_H, 4, 8)
    desc = cases.desc(binding.CAPTURE_EQUIRECT, 8, 4, cases.origins(case["name"])[0], True)

    def answers():
        return [g.radiance(case["rays"][:65], 17, EPSILON, cases.SEED), g.capture(desc, 17, EPSILON, cases.SEED)]

    before = answers()
    whole = g.process_job(cases.CAMERA, opt, base_seed=11)
    frame = binding.Frame(g, cases.CAMERA, opt, base_seed=11)
    try:
        frame.set_progressive(2, 1)
        _, _, info = frame.render()
        assert info["cancelled"]
        during = answers()
        ref.assert_records_equal(during[0], before[0], "beside a live frame: rays")
        ref.assert_records_equal(during[1], before[1], "beside a live frame: capture")
        frame.set_progressive(0)
        image, _, info = frame.render()
        assert info["status"] == binding.PT_OK
        assert_bits_equal(image, whole, "the frame after the radiance calls")
    finally:
        frame.close()


def test_the_furnace():
    """Captures at the centre of one closed sphere of triangles with diffuse (0, 0, 0, 1) and emission (0.75, 0.5, 0.25), 64 samples:
    every sample that has a ray meets a wall, its radiance is the emission and its alpha 1, the black walls add zeros behind it.  64 equal
    numbers with three significant bits sum exactly in fp32, and the division by 64 is exact."""
    scene, _ = light_probe_cases.furnace()
    e = np.asarray(light_probe_cases.FURNACE_EMISSION[:3] + (1.0,), F)
    view = ((0.0, 0.0, 0.0), (0.3, -0.2, 1.0))
    g = binding.Scene(scene)
    try:
        for label, model, width, height, kw in cases.SMALL:
            if model == binding.CAPTURE_ORTHO:
                kw = dict(extent=(0.3, 0.3))  # (the window stays inside the sphere)
            for jitter in (False, True):
                got = g.capture(cases.desc(model, width, height, view, jitter, **kw), 64, EPSILON, cases.SEED)
                inside = got["outside"] == 0
                assert inside.sum() >= 9 and (got["samples"] == 64).all()  # (a jittered 5 x 5 fisheye keeps its inner 3 x 3 wholly inside)
                assert (got["value"][inside] == e).all() and (got["missed"] == 0).all(), (label, jitter, got["value"][inside][got["value"][inside] != e])
                assert inside.all() or model == binding.CAPTURE_FISHEYE
    finally:
        g.close()


DEVICE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding
from tests import radiance_cases as cases
name = sys.argv[2]
scene, _, _ = cases.build(name)
g = binding.Scene(scene, device=0)
rng = np.random.default_rng(4)
o = rng.uniform(-0.8, 0.8, (130, 3)) + np.array([0, 0, 0.9])
d = rng.normal(size=(130, 3))
rays = np.ascontiguousarray(np.concatenate([o, d], axis=1), np.float32)
desc = cases.desc(binding.CAPTURE_FISHEYE, 9, 9, cases.origins(name)[0], True, fov=2.5)
stream = torch.cuda.current_stream(0).cuda_stream
ok = True
for s in (stream, 0):
    d_rays = torch.from_numpy(rays).to("cuda:0")
    d_out = torch.full((len(rays), 8), -7, dtype=torch.int32, device="cuda:0")
    g.radiance_device(d_rays.data_ptr(), len(rays), d_out.data_ptr(), 65, 1e-3, cases.SEED, s)
    same = d_out.cpu().numpy().view(binding.RadianceResult).ravel().tobytes() == g.radiance(rays, 65, 1e-3, cases.SEED).tobytes()
    d_img = torch.full((81, 8), -7, dtype=torch.int32, device="cuda:0")
    g.capture_device(desc, d_img.data_ptr(), 65, 1e-3, cases.SEED, s)
    same_capture = d_img.cpu().numpy().view(binding.RadianceResult).ravel().tobytes() == g.capture(desc, 65, 1e-3, cases.SEED).tobytes()
    print("rays %s, capture %s" % ("bit-identical" if same else "DIFFERENT", "bit-identical" if same_capture else "DIFFERENT"))
    ok &= same and same_capture
g.close()
sys.exit(0 if ok else 1)
"""


@pytest.mark.parametrize("name", ["S", "L"])
def test_device_forms_give_the_same_bytes(name):
    """pt_radiance_rays_device and pt_radiance_capture_device on torch's stream and on the null stream against their host forms, in a
    fresh interpreter in which torch opens the device first (tests/test_gpu_gather.py's arrangement)."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT, name], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("bit-identical") == 4, r.stdout
