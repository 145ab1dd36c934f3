"""Light probes on the GPU (include/pt_light_probes.h).  All comparisons but the furnace's are exact: pt_light_probes_points
against the yardstick tests/light_probe_ref.py on the oracle, coefficients and counts bit for bit, on scenes S (tree in LDS), L
(device-built, records in HBM, walks that outgrow the stack's LDS window) and G (glass, both emitter kinds, point lights, a one-way mirror)
with the probes of tests/light_probe_cases.py; every chunk size gives the same bits; the device forms equal the host forms; a grid's
records equal the probes at its nodes; a probe's sample is the radiance call's along the same direction, bit for bit; the
lookup equals its restatement bit for bit; after a relight the scene answers as a fresh one; a
live frame is left alone; and in a furnace the record and the lookup return the emission."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from cpupathtrace_amd import binding, scenes
from tests import gather_ref, light_probe_cases as cases, light_probe_ref as ref, pose_probe, query_cases
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EPSILON = cases.OPTIONS["epsilon"]
MOST = max(cases.SAMPLES)


@pytest.fixture(scope="module")
def assembler(tmp_path_factory):
    return pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("light_probe_pose") / "libpose_probe.so")))


@pytest.fixture(scope="module", params=["S", "L", "G"])
def case(request, oracle_lib, assembler):
    """A scene on the device and flattened for the oracle, its probes, and the yardstick's samples of all of them, computed once: sample
    s of probe i has its own engine, so the first k samples of the largest count are the samples of a call with k.  The scene is closed
    behind the module's last test of it, so that nothing of it stays on the device for the tests that follow."""
    name = request.param
    scene, instances, shapes = cases.build(name)
    flat = query_cases.flatten(scene, instances, shapes, assembler)
    handle = oracle_lib.scene_create(flat["scene"])
    pos = cases.probes(handle, flat, name)
    d, L, missed, backfacing, _ = ref.samples_of(handle, flat, pos, MOST, EPSILON, cases.SEED)
    g = binding.Scene(scene)
    yield dict(name=name, scene=scene, flat=flat, handle=handle, pos=pos, samples=(d, L, missed, backfacing), g=g, want={})
    g.close()
    handle.close()


def _want(case, samples):
    """The yardstick's records of all the case's probes at a sample count (a probe's record does not depend on how many follow it)."""
    if samples not in case["want"]:
        d, L, missed, backfacing = case["samples"]
        case["want"][samples] = ref.project(d[:, :samples], L[:, :samples], missed[:, :samples], backfacing[:, :samples])
    return case["want"][samples]


@pytest.mark.parametrize("samples", cases.SAMPLES)
def test_probes_against_the_yardstick(case, samples):
    g, want = case["g"], _want(case, samples)
    for n in cases.BATCHES:
        got = g.light_probes(case["pos"][:n], samples, EPSILON, cases.SEED)
        ref.assert_probes_equal(got, want[:n], "%s, %d probes x %d samples" % (case["name"], n, samples))
    assert (want["samples"] == samples).all() and (want["missed"] + want["backfacing"] <= samples).all()
    print("%s x %d: mean band 0 %s, missed %d, backfacing %d of %d" % (case["name"], samples, np.nanmean(want["sh"][:, 0], axis=0), want["missed"].sum(), want["backfacing"].sum(),
                                                                      samples * len(want)))


def test_an_empty_call(case):
    assert len(case["g"].light_probes(np.zeros((0, 3), F), 4, EPSILON)) == 0
    grid = binding.light_probe_grid((0, 0, 0), (1, 1, 1), (1, 1, 1))
    assert case["g"].shade_with_light_probes(grid, np.zeros(1, binding.LightProbe), np.zeros((0, 3), F), np.zeros((0, 3), F)).shape == (0, 4)


def test_chunks_change_no_bit(case):
    """PT_LIGHT_PROBE_CHUNK is read per call and counts (probe, sample) pairs: 17 holds exactly one probe of 17 samples, 64 three, 1000
    58; 1 is less than a probe: one probe per launch."""
    g, n, samples = case["g"], 65, 17
    want = _want(case, samples)[:n]
    whole = g.light_probes(case["pos"][:n], samples, EPSILON, cases.SEED)
    ref.assert_probes_equal(whole, want, "the default chunk")
    before = os.environ.get("PT_LIGHT_PROBE_CHUNK")
    try:
        for chunk in cases.CHUNKS:
            os.environ["PT_LIGHT_PROBE_CHUNK"] = str(chunk)
            got = g.light_probes(case["pos"][:n], samples, EPSILON, cases.SEED)
            ref.assert_probes_equal(got, whole, "%s, chunks of %d pairs" % (case["name"], chunk))
        # more than one strided round per probe, the cut between probes: 130 pairs hold two probes of 65 samples, 200 three (and 5 spare)
        for chunk in (130, 200):
            os.environ["PT_LIGHT_PROBE_CHUNK"] = str(chunk)
            got = g.light_probes(case["pos"][:n], 65, EPSILON, cases.SEED)
            ref.assert_probes_equal(got, _want(case, 65)[:n], "%s, 65 samples, chunks of %d pairs" % (case["name"], chunk))
        os.environ["PT_LIGHT_PROBE_CHUNK"] = "64"  # a probe that alone has more pairs gets a launch of its own
        got = g.light_probes(case["pos"][:5], 130, EPSILON, cases.SEED)
        ref.assert_probes_equal(got, _want(case, 130)[:5], "probes larger than a chunk")
    finally:
        if before is None:
            del os.environ["PT_LIGHT_PROBE_CHUNK"]
        else:
            os.environ["PT_LIGHT_PROBE_CHUNK"] = before


def _base_seed_for_state(state, x=0, y=0):
    """The base_seed whose engine RandomEngine(pt_pixel_seed(base_seed, x, y)) has `state`: both maps are bijections of 64-bit words
    (seed ^ (~seed << 32) keeps the low half; splitmix64's finaliser is xor-shifts and odd multiplications), undone step by step."""
    M = (1 << 64) - 1

    def unshift(v, s):  # the z of v = z ^ (z >> s)
        z = v
        for _ in range(64 // s + 1):
            z = v ^ (z >> s)
        return z

    lo = state & 0xFFFFFFFF
    seed = ((((state >> 32) ^ ~lo) & 0xFFFFFFFF) << 32) | lo
    z = unshift(seed, 31)
    z = unshift((z * pow(0x94D049BB133111EB, -1, 1 << 64)) & M, 27)
    z = unshift((z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & M, 30)
    base_seed = (z - 0x9E3779B97F4A7C15 * (1 + (y << 32) + x)) & M
    assert binding.seed_to_state(binding.pixel_seed(base_seed, x, y)) == state
    return base_seed


def test_a_probe_sample_is_the_radiance_along_its_direction(case):
    """The light-probe kernel against the radiance kernel, sample for sample: the yardstick's direction of a probe's one sample, a radiance
    ray from the probe along it whose engine starts where the probe's stands behind its two draws (a base_seed made for that), and the
    ray's traced rgb is that sample's L_s -- the yardstick's, and the one in the probe's record, through the yardstick's projection."""
    g, n = case["g"], 3
    pos = case["pos"][:n]
    d, states = ref.directions(gather_ref.sample_states(cases.SEED, n, 1).reshape(-1))
    assert_bits_equal(d, case["samples"][0][:n, 0], "the directions")
    L = np.zeros((n, 1, 4), F)
    missed = np.zeros((n, 1), bool)
    for i in range(n):
        ray = np.concatenate([pos[i], d[i]]).astype(F)
        rec = g.radiance(ray, 1, EPSILON, _base_seed_for_state(int(states[i])))[0]
        L[i, 0], missed[i, 0] = rec["value"], rec["missed"] == 1
        assert rec["samples"] == 1 and rec["outside"] == 0
    _, want_L, want_missed, backfacing = (v[:n, :1] for v in case["samples"])
    assert (missed == want_missed).all()
    ref.assert_floats_equal(L[:, :, :3], want_L[:, :, :3], "%s: a ray's rgb against the probe sample's L_s" % case["name"])
    got = g.light_probes(pos, 1, EPSILON, cases.SEED)
    ref.assert_probes_equal(got, ref.project(d.reshape(n, 1, 3), L, missed, backfacing), "%s: the probes' records from the rays' rgb" % case["name"])


def _grid_records(case, count, samples=64):
    key = ("grid", count, samples)
    if key not in case["want"]:
        case["want"][key] = case["g"].light_probe_grid(*cases.grid_of(case["name"], count), samples=samples, epsilon=EPSILON, base_seed=cases.SEED)
    return case["want"][key]


@pytest.mark.parametrize("count", cases.GRIDS)
def test_a_grid_is_the_probes_at_its_nodes(case, count):
    g = case["g"]
    grid, got = _grid_records(case, count)
    assert got.shape == count[::-1]
    positions = ref.grid_positions(grid)
    assert len(positions) == int(np.prod(count))
    want = g.light_probes(positions, 64, EPSILON, cases.SEED)
    ref.assert_probes_equal(got.ravel(), want, "grid %s of %s" % (count, case["name"]))
    if case["name"] == "G":
        at = 1 if count[0] > 1 else 0  # the centre of the closed box
        assert (positions[at] == np.asarray(cases.BOX_CENTRE, F)).all()
        yardstick = ref.light_probes(case["handle"], case["flat"], positions[at:at + 1], 64, EPSILON, cases.SEED)
        # (probe `at` of a call has the engines of index `at`: the yardstick's call has it at 0 -- compare through a call of its own)
        alone = g.light_probes(positions[at:at + 1], 64, EPSILON, cases.SEED)
        ref.assert_probes_equal(alone, yardstick, "the box centre")


@pytest.mark.parametrize("count", cases.GRIDS)
def test_the_lookup_is_its_restatement(case, count):
    g = case["g"]
    grid, records = _grid_records(case, count)
    records = records.ravel()
    P, N = cases.lookup_points(cases.grid_of(case["name"], count))
    for mb in (0.25, 1.0, 0.0):
        got = g.shade_with_light_probes(grid, records, P, N, mb)
        want = ref.shade(grid, records, P, N, mb)
        ref.assert_floats_equal(got, want, "lookup on grid %s of %s, max_backfacing %g" % (count, case["name"], mb))
    everything = ref.shade(grid, records, P, N, 1.0)
    assert (everything[:, 3] > 0).all() and (everything[:-3, 3] > 0.99).all()  # nothing is excluded at 1: the weights sum to 1
    if case["name"] == "G":
        # the box-centre probe is excluded by the default max_backfacing: on its node nothing is left, around it the weights sum to less
        at = 1 if count[0] > 1 else 0
        assert records["backfacing"][at] > 0.25 * records["samples"][at]
        default = ref.shade(grid, records, P, N, 0.25)
        node = 40 + at  # (lookup_points: 40 points inside, then the nodes)
        assert default[node, 3] <= 1e-5 and abs(everything[node, 3] - 1) <= 1e-6  # (a node's own coordinate may round a hair beside it)
        assert (default[:, 3] < everything[:, 3]).sum() >= (1 if count == (1, 1, 1) else 10)
    # all eight corners excluded: the zero result, everywhere
    buried = records.copy()
    buried["backfacing"] = buried["samples"]
    got = g.shade_with_light_probes(grid, buried, P, N, 0.25)
    assert (got == 0).all() and got.shape == (len(P), 4)


def test_probes_follow_a_relight(oracle_lib, assembler):
    """Scene S relit in place: the probes and a grid equal those of a scene created afresh with the new look."""
    lights = (np.array([[0.5, 0.8, -0.5]], F), np.array([[0.1, 0.2, 0.9, 1.0]], F))
    scene, instances, shapes = query_cases.build(False)
    flat = query_cases.flatten(scene, instances, shapes, assembler)
    handle = oracle_lib.scene_create(flat["scene"])
    pos = cases.probes(handle, flat, "S")[:65]
    handle.close()
    grid = cases.grid_of("S", (2, 1, 3))
    g = binding.Scene(scene)
    try:
        before = g.light_probes(pos, 17, EPSILON, cases.SEED)
        table = g.materials()
        table[query_cases.MATERIAL_INDEX["glow"]]["emission"] = (0.2, 1.0, 0.3, 3.0)
        g.relight(materials=table, point_lights=lights)
        relit, _, _ = query_cases.build(False, materials={"glow": dict(emission=(0.2, 1.0, 0.3, 3.0))})
        relit["light_pos"], relit["light_spectrum"] = lights
        fresh = binding.Scene(relit)
        try:
            after = g.light_probes(pos, 17, EPSILON, cases.SEED)
            ref.assert_probes_equal(after, fresh.light_probes(pos, 17, EPSILON, cases.SEED), "relit")
            ref.assert_probes_equal(g.light_probe_grid(*grid, samples=17, epsilon=EPSILON)[1], fresh.light_probe_grid(*grid, samples=17, epsilon=EPSILON)[1], "relit grid")
            assert after.tobytes() != before.tobytes()
            assert (after["missed"] == before["missed"]).all() and (after["backfacing"] == before["backfacing"]).all()  # the tree is untouched
        finally:
            fresh.close()
    finally:
        g.close()


def test_light_probes_leave_a_live_frame_alone(case):
    """A progressive frame stopped after its first pass, light probe calls of every kind in between: the frame finishes as process_job
    renders it, and the calls answer as without it."""
    g = case["g"]
    opt = scenes.options(cases.FRAME_W, cases.FRAME_H, 4, 8)
    pos = case["pos"][:65]
    grid = cases.grid_of(case["name"], (2, 1, 3))
    P, N = cases.lookup_points(grid)

    def answers():
        records = g.light_probes(pos, 17, EPSILON, cases.SEED)
        grid_, nodes = g.light_probe_grid(*grid, samples=17, epsilon=EPSILON, base_seed=cases.SEED)
        return [records, nodes.ravel(), g.shade_with_light_probes(grid_, nodes, P, N)]

    before = answers()
    whole = g.process_job(cases.CAMERA, opt, base_seed=11)
    frame = binding.Frame(g, cases.CAMERA, opt, base_seed=11)
    try:
        frame.set_progressive(2, 1)
        _, _, info = frame.render()
        assert info["cancelled"]
        during = answers()
        ref.assert_probes_equal(during[0], before[0], "beside a live frame: probes")
        ref.assert_probes_equal(during[1], before[1], "beside a live frame: grid")
        ref.assert_floats_equal(during[2], before[2], "beside a live frame: lookup")
        frame.set_progressive(0)
        image, _, info = frame.render()
        assert info["status"] == binding.PT_OK
        assert_bits_equal(image, whole, "the frame after the light probes")
    finally:
        frame.close()


def test_the_furnace(oracle_lib):
    """A probe at the centre of one closed sphere of triangles with diffuse (0, 0, 0, 1) and emission e, 1024 samples.  On the yardstick
    every L_s is exactly e (tests/test_light_probes_cpu.py checks it there as well), so the band-0 sum is e times a sum of 1024 equal
    numbers: each of its 1024 fp32 additions is within 2^-24 relative."""
    scene, flat = cases.furnace()
    e = np.asarray(cases.FURNACE_EMISSION[:3], np.float64)
    n = cases.FURNACE_SAMPLES
    handle = oracle_lib.scene_create(flat["scene"])
    d, L, missed, backfacing, _ = ref.samples_of(handle, flat, [[0.0, 0.0, 0.0]], n, EPSILON, cases.SEED)
    handle.close()
    assert (L[0, :, :3] == e.astype(F)).all() and not missed.any() and backfacing.all()
    g = binding.Scene(scene)
    try:
        got = g.light_probes([[0.0, 0.0, 0.0]], n, EPSILON, cases.SEED)
        ref.assert_probes_equal(got, ref.project(d, L, missed, backfacing), "the furnace")
        assert got["samples"][0] == n and got["missed"][0] == 0 and got["backfacing"][0] == n
        sh = got["sh"][0].astype(np.float64)
        band0 = 0.282095 * 4 * math.pi * e
        print("furnace: sh[0] / (0.282095 4 pi e) - 1 = %s, max |sh[k >= 1]| / e = %s against %.4f" % (sh[0] / band0 - 1, np.abs(sh[1:] / e).max(axis=0), 6 * math.sqrt(4 * math.pi / n)))
        assert (np.abs(sh[0] - band0) <= n * 2.0 ** -24 * band0).all()
        assert (np.abs(sh[1:]) <= 6 * e * math.sqrt(4 * math.pi / n)).all()
        # the lookup on a 1 x 1 x 1 grid of that probe returns e for any N: band 0 gives 0.282095^2 4 pi e within the bound above, every
        # other band at most a_k |Y_k(N)| times its bound, and the evaluation's own roundings (at most 16 per term) are below 2^-19 of the
        # terms' sizes; max_backfacing 1 keeps the probe, which sees every wall from behind
        grid = binding.light_probe_grid((0, 0, 0), (1, 1, 1), (1, 1, 1))
        rng = np.random.default_rng(2)
        N = rng.normal(size=(64, 3))
        N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
        P = rng.uniform(-3, 3, (64, 3)).astype(F)
        value = g.shade_with_light_probes(grid, got, P, N, 1.0)
        ref.assert_floats_equal(value, ref.shade(grid, got, P, N, 1.0), "the furnace's lookup")
        assert (value[:, 3] == 1).all()
        aY = np.abs(ref.A.astype(np.float64) * ref.basis(N).astype(np.float64))
        centre = 0.282095 ** 2 * 4 * math.pi
        others = aY[:, 1:].sum(axis=1)[:, None] * 6 * math.sqrt(4 * math.pi / n)
        bound = (abs(centre - 1) + centre * n * 2.0 ** -24 + others) * e[None, :]
        bound = bound + 2.0 ** -19 * (centre + others) * e[None, :]
        assert (np.abs(value[:, :3] - e) <= bound).all(), (np.abs(value[:, :3] - e) / bound).max()
        assert (g.shade_with_light_probes(grid, got, P, N, 0.25) == 0).all()  # ... and the default drops it: the zero result
    finally:
        g.close()


DEVICE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding
from tests import light_probe_cases as cases
name = sys.argv[2]
scene, _, _ = cases.build(name)
g = binding.Scene(scene, device=0)
rng = np.random.default_rng(4)
pos = np.ascontiguousarray(rng.uniform(-0.8, 0.8, (130, 3)) + np.array([0, 0, 0.9]), np.float32)
grid, nodes = g.light_probe_grid(*cases.grid_of(name, (3, 4, 2)), samples=17, epsilon=1e-3, base_seed=cases.SEED)
P, N = cases.lookup_points(cases.grid_of(name, (3, 4, 2)))
pts = np.ascontiguousarray(np.concatenate([P, N], axis=1), np.float32)
stream = torch.cuda.current_stream(0).cuda_stream
ok = True
for s in (stream, 0):
    d_pos = torch.from_numpy(pos).to("cuda:0")
    d_out = torch.full((len(pos), 32), -7, dtype=torch.int32, device="cuda:0")
    g.light_probes_device(d_pos.data_ptr(), len(pos), d_out.data_ptr(), 65, 1e-3, cases.SEED, s)
    same = d_out.cpu().numpy().view(binding.LightProbe).ravel().tobytes() == g.light_probes(pos, 65, 1e-3, cases.SEED).tobytes()
    d_nodes = torch.from_numpy(nodes.ravel().view(np.uint8).reshape(-1, 128)).to("cuda:0")
    d_pts = torch.from_numpy(pts).to("cuda:0")
    d_val = torch.full((len(pts), 4), -7.0, dtype=torch.float32, device="cuda:0")
    g.shade_with_light_probes_device(grid, d_nodes.data_ptr(), d_pts.data_ptr(), len(pts), d_val.data_ptr(), 0.25, s)
    same_lookup = d_val.cpu().numpy().tobytes() == g.shade_with_light_probes(grid, nodes, P, N, 0.25).tobytes()
    print("probes %s, lookup %s" % ("bit-identical" if same else "DIFFERENT", "bit-identical" if same_lookup else "DIFFERENT"))
    ok &= same and same_lookup
g.close()
sys.exit(0 if ok else 1)
"""


@pytest.mark.parametrize("name", ["S", "L"])
def test_device_forms_give_the_same_bytes(name):
    """pt_light_probes_points_device and pt_light_probes_shade_device on torch's stream and on the null stream against their host forms,
    in a fresh interpreter in which torch opens the device first (tests/test_gpu_gather.py's arrangement)."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT, name], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("bit-identical") == 4, r.stdout
