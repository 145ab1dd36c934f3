"""The rare step of the traversal (Tracer::slow_step: leaf test, what follows a hit, pop loop) as straight-line code, on the GPU.

(a) tri_intersect of pt_device.h through the unit probe against the C oracle, bit for bit, on the edge vectors of tests/slow_step_cases.py
    (tests/test_slow_step_cases_cpu.py holds the oracle equal to the compiled reference on the same arrays).
(b) Scheduling invariance, after tests/test_gpu_refill.py: PT_LEAF_MIN decides how many lanes must wait before the rare step runs -- WHEN a leaf
    is tested and a walk pops, never which.  1 runs it in every step for a single lane; 64 (with bursts of one step) only when no lane stands on
    an inner node any more, for all the waiting lanes at once.  Each case renders the same frame bit for bit as the default settings, counts
    the same rays, node visits, leaf tests, samples and vertices, and shows in wave_steps / shading_passes that its setting was applied; at
    most 64 pixels per scene go through the CPU oracle.  The knobs are held for scene creation + render (tests.util.env).
(c) A scene whose walks park more nodes than the stack window holds, so that the pop loop brings entries back from the spill area: every
    pixel against the oracle."""
import numpy as np
import pytest

import oracle
from cpupathtrace_amd import binding, scenes
from tests import slow_step_cases as sc
from tests.test_gpu_refill import SCHEDULE_STATS, SEED, WORK_STATS, _against_oracle, _moved, _render, _same_work, _scene
from tests.util import assert_bits_equal


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe():
    from tests import unit_probe
    p = unit_probe.Probe()
    if p.device_count() < 1:
        pytest.fail("no HIP device: the unit probe has no CPU path")
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("family", [name for name, _ in sc.FAMILIES])
def test_tri_intersect_edge_vectors(probe, oracle_lib, family):
    tri, cull, rays = sc.edge_vectors()[family]
    want = oracle_lib.tri_intersect(tri, cull, rays)
    assert_bits_equal(probe.tri_intersect(tri, cull, rays), want, "tri_intersect, %s" % family)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------

# scene, width, height, spp, what is set with every render of the case, step of the oracle's pixel grid
# (lit_room at 32 x 32 has ONE slot per wavefront, where a waiting lane changes nothing a counter shows: its streams go to 16 wavefronts, as in
# tests/test_gpu_refill.py)
CASES = [
    ("box", 64, 64, 4, {}, 8),
    ("dragonbox", 96, 96, 8, {}, 12),
    ("lit_room", 32, 32, 4, {"PT_SPREAD_WAVES": 16}, 4),
    ("cornell", 64, 64, 4, {}, 8),
    ("cornell", 64, 64, 4, {"PT_STACK_WINDOW": 4}, 8),
]
VARIANTS = [{"PT_LEAF_MIN": 1}, {"PT_LEAF_MIN": 64, "PT_BURST": 1}]


def _ids(v):
    if isinstance(v, dict):
        return ",".join("%s=%s" % (k[3:].lower(), x) for k, x in v.items()) or "plain"
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,spp,held,oracle_step", CASES, ids=_ids)
def test_leaf_min_moves_the_schedule_only(oracle_lib, name, w, h, spp, held, oracle_step):
    desc, cam = _scene(name)
    opt = scenes.options(w, h, spp, spp)
    want, st0 = _render(desc, cam, opt, **held)
    print("%s %s: default %s" % (name, held, {k: st0[k] for k in WORK_STATS + SCHEDULE_STATS}))
    assert st0["samples"] == w * h * spp and st0["rays_traced"] > st0["shadow_rays_traced"] > 0 and st0["leaf_tests"] > 0
    if held:
        plain, st_plain = _render(desc, cam, opt)
        assert_bits_equal(want, plain, "%s: frame under %s" % (name, held))
        _same_work(st_plain, st0, (name, held))
    for knobs in VARIANTS:
        got, st1 = _render(desc, cam, opt, **dict(held, **knobs))
        print("%s %s: %s" % (name, knobs, {k: st1[k] for k in WORK_STATS + SCHEDULE_STATS}))
        assert_bits_equal(got, want, "%s: frame under %s" % (name, knobs))
        _same_work(st0, st1, (name, knobs))
        assert _moved(st0, st1), "%s: %s changed neither wave_steps nor shading_passes (%s)" % (name, knobs, st1)
    _against_oracle(oracle_lib, desc, cam, opt, want, oracle_step)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------

DEEP_TRIANGLES = 1500  # (+ the two of the emitter)
DEEP_CAMERA = scenes.camera((0, 0, -3), (0, 0, 0.5), (0, 1, 0), 1.5, 1.0, -1.0)  # the frame is the square [-1, 1]^2 at z = 0


def _deep_stack_scene():
    """1500 large triangles stacked along the view direction: each spans most of [-1, 1]^2 in x and y (its corners lie near three of the
    square's four corners), tilted by up to 0.3 in z about a height between 0 and 1, in one of 8 colours; an emissive quad behind the camera lights them.

    Why walks park more than the 8 nodes of the stack window: every triangle's box -- hence every box of the tree -- covers the middle of the
    square over a range of z that holds the triangle's height, so a ray from the camera through the middle of the frame enters BOTH children
    of every inner node it meets until its first hit shortens the pruning distance; on that first descent the far child is parked at every
    level, and the walk stands on a leaf of depth D with D + 1 entries on its stack (the sentinel included).  A binary tree has at most 256
    leaves of depth <= 8, so at least five in six of the 1500 leaves lie deeper, whatever the builder does: D + 1 >= 10 > 8, the oldest
    entries are in the spill area, and the pops that follow the hit bring them back into the window one by one -- most of them only to be
    discarded, their entry distance no longer below the pruning distance.  (The oracle reports no stack depth.  What it does report, and
    test_deep_stack_scene_overlaps checks without a GPU: the rays of the middle pixels test many triangles each, which they can only do
    by entering both children and returning to the parked one over and over.)"""
    rng = np.random.default_rng(77)
    n = DEEP_TRIANGLES
    corners = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64)
    pick = np.stack([(k - np.arange(3)) % 4 for k in rng.integers(0, 4, n)])  # (clockwise seen from +z: the faces look at the camera)
    xy = corners[pick] * rng.uniform(0.8, 1.0, (n, 3, 1)) + rng.uniform(-0.1, 0.1, (n, 3, 2))
    z = rng.uniform(0.0, 1.0, (n, 1)) + rng.uniform(-0.3, 0.3, (n, 3))
    tri = np.concatenate([xy, z[:, :, None]], axis=2).astype(np.float32)
    sb = scenes.SceneBuilder()
    for k in range(8):
        colour = (0.3 + 0.1 * (k & 1) + 0.2 * ((k >> 1) & 1), 0.9 - 0.1 * k, 0.25 + 0.09 * k, 1.0)
        sb.triangles(tri[k::8], sb.material(colour))
    sb.triangles(scenes.make_plane((-1.5, -1.5, -3.5), (1.5, 1.5, -3.5)), sb.material((1, 1, 1, 1), 1.0, (4, 3.5, 3, 1)))
    return sb.build(), DEEP_CAMERA


def _middle_pixels(w, h, half):
    ys, xs = np.mgrid[h // 2 - half:h // 2 + half, w // 2 - half:w // 2 + half]
    return xs.ravel().astype(np.int32), ys.ravel().astype(np.int32)


def test_deep_stack_scene_overlaps(oracle_lib):
    """CPU, by the oracle's own counters: a walk tests one leaf more for every node at which it entered both children and later returned to the
    parked one, so a scene query that tests more than 9 triangles on average has parked, and popped back, more than 8 nodes per walk."""
    desc, cam = _deep_stack_scene()
    opt = scenes.options(32, 32, 2, 2)
    xs, ys = _middle_pixels(32, 32, 3)
    states = np.array([binding.seed_to_state(binding.pixel_seed(SEED, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
    handle = oracle_lib.scene_create(desc)
    try:
        handle.counters_reset()
        handle.render_streams(cam, opt, oracle.pixel_streams(xs, ys, states), n_threads=4)
        c = handle.counters()
    finally:
        handle.close()
    print(c)
    assert c["samples"] == len(xs) * 2 and c["scene_queries"] >= c["samples"]
    assert c["tri_tests"] > 9 * c["scene_queries"], c


@pytest.mark.gpu
def test_deep_stack_pops_through_the_spill_area(oracle_lib):
    """(c): 32 x 32 x 4 at the default window of 8 entries, every pixel against the oracle; the tree is as deep as the argument of
    _deep_stack_scene needs, and the kernel's counters stand to the oracle's as in tests/test_gpu_parity.py (extension rays equal; a shadow walk
    stops at its first occluder, so its tests are bounded by the oracle's)."""
    desc, cam = _deep_stack_scene()
    w = h = 32
    opt = scenes.options(w, h, 4, 4)
    scene = binding.Scene(desc)
    try:
        info = scene.info()
        img, st = scene.process_job(cam, opt, base_seed=SEED, want_stats=True)
    finally:
        scene.close()
    print(info, {k: st[k] for k in WORK_STATS + SCHEDULE_STATS})
    assert info["depth"] >= 11, info  # 1500 leaves: no binary tree is shallower
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.ravel().astype(np.int32), ys.ravel().astype(np.int32)
    states = np.array([binding.seed_to_state(binding.pixel_seed(SEED, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
    handle = oracle_lib.scene_create(desc)
    try:
        handle.counters_reset()
        want, _ = handle.render_streams(cam, opt, oracle.pixel_streams(xs, ys, states), n_threads=8)
        c = handle.counters()
    finally:
        handle.close()
    assert_bits_equal(img, want, "deep-stack frame against the oracle")
    assert (img[..., :3] > 0).any(axis=2).mean() > 0.5  # (the frame is lit: equal bits mean something)
    assert st["samples"] == c["samples"] == w * h * 4
    assert st["vertices"] == c["vertices"] > 0
    assert st["rays_traced"] - st["shadow_rays_traced"] == c["scene_queries"] - c["shadow_rays"]
    assert 0 < st["shadow_rays_traced"] <= c["shadow_rays"]
    assert st["leaf_tests"] <= c["tri_tests"] and 2 * st["node_visits"] + st["rays_traced"] <= c["aabb_tests"]
