"""Light-group passes on the GPU (include/pt_light_passes.h).  Every comparison of passes is exact: pt_light_passes_rays
and pt_light_passes_capture against the yardstick tests/light_pass_ref.py on the oracle, bit for bit, on scene G with the tables and rays of
tests/light_pass_cases.py; `total` is the radiance call's record byte for byte; every chunk size gives the same bits; the table's counts
are checked against the scene's, also behind a relight; the mix on the device is the numpy restatement; the device forms equal the host
forms; a live frame is left alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cpupathtrace_amd import binding, scenes
from tests import light_pass_cases as cases, light_pass_ref as ref, pose_probe, query_cases, radiance_cases, radiance_ref
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
EPSILON = cases.OPTIONS["epsilon"]
MOST = max(cases.SAMPLES)
CAPTURE_SAMPLES = [1, 65]


@pytest.fixture(scope="module")
def assembler(tmp_path_factory):
    return pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("light_pass_pose") / "libpose_probe.so")))


@pytest.fixture(scope="module")
def case(oracle_lib, assembler):
    """Scene G on the device and flattened for the oracle, the case rays, and the yardstick's terms of all of them at the largest sample
    count, computed once: sample s of ray i has its own engine, so the first k samples are the samples of a call with k."""
    scene, instances, shapes = cases.build()
    flat = query_cases.flatten(scene, instances, shapes, assembler)
    handle = oracle_lib.scene_create(flat["scene"])
    rays = cases.rays(flat)
    L, missed, terms = ref.ray_terms(handle, flat, rays, MOST, EPSILON, cases.SEED)
    g = binding.Scene(scene)
    yield dict(scene=scene, flat=flat, handle=handle, rays=rays, L=L, missed=missed, terms=terms, g=g, want={}, count={})
    g.close()
    handle.close()


def _want(case, name, split, samples):
    """The yardstick's pass records of all the case's rays for a table at a sample count, and the most non-zero terms of a sample."""
    key = (name, split, samples)
    if key not in case["want"]:
        terms = ref.first_samples(case["terms"], MOST, samples)
        acc, count = ref.accumulate(terms, len(case["rays"]) * samples, cases.table(name, split))
        case["want"][key], case["count"][key] = ref.pass_records(acc, samples), int(count.max())
    return case["want"][key]


def _total(case, samples):
    return radiance_ref.records(case["L"][:, :samples], case["missed"][:, :samples])


@pytest.mark.parametrize("samples", cases.SAMPLES)
@pytest.mark.parametrize("name,split", cases.TABLES, ids=["%s-%d" % t for t in cases.TABLES])
def test_passes_against_the_yardstick(case, name, split, samples):
    g, want, groups = case["g"], _want(case, name, split, samples), cases.groups(cases.table(name, split))
    for n in cases.BATCHES + [cases.N_RAYS]:
        passes, total = g.light_passes(case["rays"][:n], groups, samples, EPSILON, cases.SEED)
        ref.assert_passes_equal(passes, want[:n], "%s split %d, %d rays x %d samples" % (name, split, n, samples))
        radiance_ref.assert_records_equal(total, _total(case, samples)[:n], "total")
    assert (want["value"] != 0).any(axis=(0, 2)).sum() >= (8 if split else 3)
    # without a total the passes are the same
    passes, none = g.light_passes(case["rays"], groups, samples, EPSILON, cases.SEED, want_total=False)
    assert none is None
    ref.assert_passes_equal(passes, want, "without a total")


def test_an_empty_call(case):
    passes, total = case["g"].light_passes(np.zeros((0, 6), F), cases.groups(cases.table("THREE", True)), 4, EPSILON)
    assert passes.shape == (0, 9) and total.shape == (0,)


@pytest.mark.parametrize("split", [False, True])
def test_total_is_the_radiance_call_byte_for_byte(case, split):
    g, groups = case["g"], cases.groups(cases.table("EIGHT", split))
    for samples in (1, 65):
        _, total = g.light_passes(case["rays"], groups, samples, EPSILON, cases.SEED)
        assert total.tobytes() == g.radiance(case["rays"], samples, EPSILON, cases.SEED).tobytes()
    for label, model, width, height, kw in radiance_cases.SMALL:
        desc = radiance_cases.desc(model, width, height, radiance_cases.origins("G")[0], True, **kw)
        _, total = g.capture_light_passes(desc, groups, 17, EPSILON, cases.SEED)
        assert total.tobytes() == g.capture(desc, 17, EPSILON, cases.SEED).tobytes(), label


def test_one_group_is_the_total_at_one_sample(case):
    """One group, no split, samples = 1: the single accumulator takes the terms the ordinary one takes, in its order, and a record of one
    sample is that sample."""
    one = binding.light_groups(1, np.zeros(len(cases.MATERIALS), np.uint8), np.zeros(cases.N_POINT_LIGHTS, np.uint8))
    passes, total = case["g"].light_passes(case["rays"], one, 1, EPSILON, cases.SEED)
    assert passes.shape == (cases.N_RAYS, 1)
    a, b = np.ascontiguousarray(passes["value"][:, 0]), np.ascontiguousarray(total["value"][:, :3])
    assert ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    assert (a != 0).any()


def test_chunks_change_no_bit(case):
    """PT_RADIANCE_CHUNK is read per call; a launch holds PT_RADIANCE_CHUNK / P pairs, P = 9 here: with 17 samples 1, 17, 64 and 130 are
    less than one ray's share (one ray per launch: a ray that alone exceeds a chunk), 200 holds one ray, 1000 six; with 65 samples 1000
    holds one ray."""
    g, n, groups = case["g"], 65, cases.groups(cases.table("THREE", True))
    before = os.environ.get("PT_RADIANCE_CHUNK")
    try:
        for samples in (17, 65):
            os.environ.pop("PT_RADIANCE_CHUNK", None)
            whole, whole_total = g.light_passes(case["rays"][:n], groups, samples, EPSILON, cases.SEED)
            ref.assert_passes_equal(whole, _want(case, "THREE", True, samples)[:n], "the default chunk")
            for chunk in cases.CHUNKS + [9 * 17 * 3, 9 * 65 * 2 + 5]:
                os.environ["PT_RADIANCE_CHUNK"] = str(chunk)
                got, total = g.light_passes(case["rays"][:n], groups, samples, EPSILON, cases.SEED)
                ref.assert_passes_equal(got, whole, "%d samples, chunks of %d" % (samples, chunk))
                assert total.tobytes() == whole_total.tobytes()
        desc = radiance_cases.desc(binding.CAPTURE_CUBE, 18, 3, radiance_cases.origins("G")[0], True)
        os.environ.pop("PT_RADIANCE_CHUNK", None)
        whole, whole_total = g.capture_light_passes(desc, groups, 17, EPSILON, cases.SEED)
        for chunk in (1, 200, 1000):
            os.environ["PT_RADIANCE_CHUNK"] = str(chunk)
            got, total = g.capture_light_passes(desc, groups, 17, EPSILON, cases.SEED)
            ref.assert_passes_equal(got, whole, "a capture in chunks of %d" % chunk)
            assert total.tobytes() == whole_total.tobytes()
    finally:
        if before is None:
            os.environ.pop("PT_RADIANCE_CHUNK", None)
        else:
            os.environ["PT_RADIANCE_CHUNK"] = before


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("label,model,width,height,kw", radiance_cases.SMALL, ids=[c[0] for c in radiance_cases.SMALL])
def test_captures_against_the_yardstick(case, label, model, width, height, kw, jitter):
    g, table = case["g"], cases.table("THREE", True)
    groups = cases.groups(table)
    for view in radiance_cases.origins("G"):
        desc = radiance_cases.desc(model, width, height, view, jitter, **kw)
        most = max(CAPTURE_SAMPLES)
        L, missed, outside, terms = ref.capture_terms(case["handle"], case["flat"], desc, most, EPSILON, cases.SEED)
        for samples in CAPTURE_SAMPLES:
            acc, _ = ref.accumulate(ref.first_samples(terms, most, samples), width * height * samples, table)
            want = ref.pass_records(acc, samples).reshape(height, width, 9)
            want_total = radiance_ref.records(L[:, :samples], missed[:, :samples], outside[:, :samples]).reshape(height, width)
            got, total = g.capture_light_passes(desc, groups, samples, EPSILON, cases.SEED)
            ref.assert_passes_equal(got, want, "%s from %s, jitter %d, %d samples" % (label, view[0], jitter, samples))
            radiance_ref.assert_records_equal(total, want_total, "total of %s" % label)
        if model == binding.CAPTURE_FISHEYE:
            # a fisheye's outside samples leave zeros in every pass and are counted in total.outside
            nothing = total["outside"] == samples
            assert nothing[[0, 0, 4, 4], [0, 4, 0, 4]].all() == (not jitter) and (total["outside"] > 0).sum() >= 4
            assert (got["value"][nothing].view(np.uint32) == 0).all() and (want["value"][nothing] == 0).all()
            assert (got["value"][total["outside"] == 0] != 0).any()


def test_the_counts_are_checked_under_the_lock(case):
    """A table of the wrong length is refused and the scene renders as before; after a relight that changes the material count the old
    table is refused and a new one works."""
    scene, _, _ = cases.build()
    g = binding.Scene(scene)
    try:
        t = cases.table("THREE", True)
        good = cases.groups(t)
        before, before_total = g.light_passes(case["rays"][:65], good, 17, EPSILON, cases.SEED)
        ref.assert_passes_equal(before, _want(case, "THREE", True, 17)[:65], "a second scene")
        for materials, lights in ((t["material_group"][:-1], t["point_light_group"]), (np.append(t["material_group"], 0), t["point_light_group"]),
                                  (t["material_group"], t["point_light_group"][:1]), (t["material_group"], np.append(t["point_light_group"], 0))):
            with pytest.raises(binding.PtError, match="do not fit the scene"):
                g.light_passes(case["rays"][:65], binding.light_groups(3, materials, lights, True), 17, EPSILON, cases.SEED)
            desc = radiance_cases.desc(binding.CAPTURE_EQUIRECT, 8, 4, radiance_cases.origins("G")[0], True)
            with pytest.raises(binding.PtError, match="do not fit the scene"):
                g.capture_light_passes(desc, binding.light_groups(3, materials, lights, True), 17, EPSILON, cases.SEED)
        again, again_total = g.light_passes(case["rays"][:65], good, 17, EPSILON, cases.SEED)
        assert again.tobytes() == before.tobytes() and again_total.tobytes() == before_total.tobytes()
        # a new look with one more material (an unused one) and one point light fewer
        materials = np.concatenate([scene["materials"], scene["materials"][:1]])
        g.relight(materials=materials, point_lights=(scene["light_pos"][:1], scene["light_spectrum"][:1]))
        with pytest.raises(binding.PtError, match="do not fit the scene"):
            g.light_passes(case["rays"][:65], good, 17, EPSILON, cases.SEED)
        fresh = binding.light_groups(3, np.append(t["material_group"], 0), t["point_light_group"][:1], True)
        passes, total = g.light_passes(case["rays"][:65], fresh, 17, EPSILON, cases.SEED)
        assert total.tobytes() == g.radiance(case["rays"][:65], 17, EPSILON, cases.SEED).tobytes()
        assert (passes["value"] != 0).any(axis=(0, 2)).reshape(3, 3).tolist() == [[True] * 3, [True] * 3, [False, True, True]]
    finally:
        g.close()


MIX_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding
from tests import light_pass_cases as cases, light_pass_ref as ref
scene, _, _ = cases.build()
g = binding.Scene(scene, device=0)
rng = np.random.default_rng(4)
o = rng.uniform(-0.8, 0.8, (130, 3)) + np.array([0, 0, 0.9])
rays = np.ascontiguousarray(np.concatenate([o, rng.normal(size=(130, 3))], axis=1), np.float32)
desc = binding.capture_desc(binding.CAPTURE_FISHEYE, 9, 9, (0.0, 0.0, 0.3), (0.1, 0.0, 1.0), (0, 1, 0), fov=2.5)
stream = torch.cuda.current_stream(0).cuda_stream
ok = True
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")
def host(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)
for name, split in (("THREE", True), ("EIGHT", False)):
    groups = cases.groups(cases.table(name, split))
    P = groups.n_passes
    passes, total = g.light_passes(rays, groups, 65, 1e-3, cases.SEED)
    image, image_total = g.capture_light_passes(desc, groups, 65, 1e-3, cases.SEED)
    gains = rng.uniform(0, 2, (P, 3)).astype(np.float32)
    for s in (stream, 0):
        d_rays = dev(rays)
        d_passes, d_total = dev(np.full(130 * P * 16, 0xF9, np.uint8)), dev(np.full(130 * 32, 0xF9, np.uint8))
        g.light_passes_device(d_rays.data_ptr(), 130, groups, d_passes.data_ptr(), d_total.data_ptr(), 65, 1e-3, cases.SEED, s)
        same = host(d_passes, binding.LightPass, (130, P)).tobytes() == passes.tobytes() and host(d_total, binding.RadianceResult, (130,)).tobytes() == total.tobytes()
        d_only = dev(np.full(130 * P * 16, 0xF9, np.uint8))
        g.light_passes_device(d_rays.data_ptr(), 130, groups, d_only.data_ptr(), 0, 65, 1e-3, cases.SEED, s)
        same &= host(d_only, binding.LightPass, (130, P)).tobytes() == passes.tobytes()
        d_image, d_image_total = dev(np.full(81 * P * 16, 0xF9, np.uint8)), dev(np.full(81 * 32, 0xF9, np.uint8))
        g.capture_light_passes_device(desc, groups, d_image.data_ptr(), d_image_total.data_ptr(), 65, 1e-3, cases.SEED, s)
        same_capture = host(d_image, binding.LightPass, (9, 9, P)).tobytes() == image.tobytes() and host(d_image_total, binding.RadianceResult, (9, 9)).tobytes() == image_total.tobytes()
        # the mix on the device, straight from the device form's passes, with and without the total
        d_gains, d_out = dev(gains), dev(np.full(130 * 16, 0xF9, np.uint8))
        g.mix_light_passes_device(d_passes.data_ptr(), 130, P, d_gains.data_ptr(), d_out.data_ptr(), d_total.data_ptr(), s)
        want = ref.mix(passes, gains, total)
        got = host(d_out, np.float32, (130, 4))
        same_mix = ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all()
        g.mix_light_passes_device(d_passes.data_ptr(), 130, P, d_gains.data_ptr(), d_out.data_ptr(), 0, s)
        want = ref.mix(passes, gains)
        got = host(d_out, np.float32, (130, 4))
        same_mix &= ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all() and (got[:, 3] == 0).all()
        print("rays %s, capture %s, mix %s" % tuple("bit-identical" if x else "DIFFERENT" for x in (same, same_capture, same_mix)))
        ok &= bool(same and same_capture and same_mix)
g.close()
sys.exit(0 if ok else 1)
"""


def test_device_forms_and_the_device_mix_give_the_same_bytes():
    """pt_light_passes_rays_device, pt_light_passes_capture_device and pt_light_passes_mix_device on torch's stream and on the null stream
    against the host forms and the numpy mix, in a fresh interpreter in which torch opens the device first (tests/test_gpu_radiance.py's
    arrangement)."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", MIX_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("bit-identical") == 12, r.stdout


def test_the_mix_of_traced_passes(case):
    """On passes the device traced: the host mix is the numpy restatement bit for bit; with gains of 1 it stays within the CPU test's
    bound of `total`; with the gain of one group 0 and the others 1 it equals the mix of the remaining passes."""
    g, samples = case["g"], 65
    for name, split in cases.TABLES:
        t = cases.table(name, split)
        passes, total = g.light_passes(case["rays"], cases.groups(t), samples, EPSILON, cases.SEED)
        P = passes.shape[1]
        rng = np.random.default_rng(P)
        gains = rng.uniform(0, 3, (P, 3)).astype(F)
        got, want = binding.mix_light_passes(passes, gains, total), ref.mix(passes, gains, total)
        assert ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all()
        assert (got[:, 3] == total["value"][:, 3]).all()
        # gains of 1: the sum of the passes in fp32, against the CPU test's bound as it stands (tests/test_light_passes_cpu.py derives it)
        _want(case, name, split, samples)
        T = case["count"][(name, split, samples)]
        ones = binding.mix_light_passes(passes, np.ones((P, 3), F), total)[:, :3].astype(D)
        value = total["value"][:, :3].astype(D)
        bound = ref.sum_bound(T, samples)
        worst = (np.abs(ones - value) / np.where(value > 0, value, 1.0)).max()
        print("%s split %d: T = %d, mix with gains of 1 against total: worst relative difference %.3g, bound %.3g" % (name, split, T, worst, bound))
        assert (np.abs(ones - value) <= bound * value).all()
        # one group switched off: its passes contribute +0 * value = +0, and adding +0 changes no bit
        C = 3 if split else 1
        for group in range(t["n_groups"]):
            off = np.ones((P, 3), F)
            off[group * C:(group + 1) * C] = 0.0
            rest = [p for p in range(P) if p // C != group]
            a = binding.mix_light_passes(passes, off, total)
            b = binding.mix_light_passes(np.ascontiguousarray(passes[:, rest]), np.ones((len(rest), 3), F), total) if rest else None
            assert b is None or a.tobytes() == b.tobytes(), (name, split, group)


def test_light_pass_calls_leave_a_live_frame_alone(case):
    """A progressive frame stopped after its first pass, calls of both kinds in between: the frame finishes as process_job renders it,
    and the calls answer as without it."""
    g, groups = case["g"], cases.groups(cases.table("THREE", True))
    opt = scenes.options(radiance_cases.FRAME_W, radiance_cases.FRAME_H, 4, 8)
    desc = radiance_cases.desc(binding.CAPTURE_EQUIRECT, 8, 4, radiance_cases.origins("G")[0], True)

    def answers():
        return [x.tobytes() for x in g.light_passes(case["rays"][:65], groups, 17, EPSILON, cases.SEED) + g.capture_light_passes(desc, groups, 17, EPSILON, cases.SEED)]

    before = answers()
    whole = g.process_job(radiance_cases.CAMERA, opt, base_seed=11)
    frame = binding.Frame(g, radiance_cases.CAMERA, opt, base_seed=11)
    try:
        frame.set_progressive(2, 1)
        _, _, info = frame.render()
        assert info["cancelled"]
        assert answers() == before
        frame.set_progressive(0)
        image, _, info = frame.render()
        assert info["status"] == binding.PT_OK
        assert_bits_equal(image, whole, "the frame after the light-pass calls")
    finally:
        frame.close()
