"""The path kernel's hand-out (retire -> pass trigger -> hand-out -> start -> window reload) at the smallest shapes at which it can go
wrong, under settings that make it run as often and as oddly as it can.  How a wavefront schedules its work decides WHEN a ray is walked,
never which: every case renders the same frame bit for bit as the same scene at default settings, counts the same rays, node visits, leaf
tests, samples and vertices (the ray counters are wavefront totals taken from the hand-out's own lane mask and from the rays a pass
queues), and shows in wave_steps / shading_passes that its setting was applied.  One case per instantiation of the kernel also compares 64
pixels with the CPU oracle.

The knobs are set in the environment for the whole of scene creation + render (tests.util.env): some are read when a scene is created,
others per job at render time.

Small jobs are spread over up to 1024 wavefronts (PT_SPREAD_WAVES), which decides what a knob can show at these sizes:
  * at 96 x 96 a wavefront has a single row of slots whatever PT_ROWS says (9216 streams, 9 slots per wavefront), so PT_ROWS=1 alone would
    move no scheduling statistic and leave most of the ring unused; that case also sets PT_SPREAD_WAVES=16, which gives every wavefront a
    FULL row: the ring of 64 x 3 rays fills up and wraps every pass or two;
  * at 32 x 32 and at 8 x 8 every wavefront has ONE slot: it takes all the rays of its only stream at once and steps until the last of them
    is back, whatever the burst length and the refill threshold are -- wave_steps and shading_passes cannot move (measured: 134347 / 17507
    and 47220 / 2090 with and without the knobs).  Those cases put their streams into few wavefronts with PT_SPREAD_WAVES (16 slots per
    wavefront at 8 x 8: still fewer than lanes, a ring that never holds 64 rays) and render once more with that alone, so that the knob under
    test is seen to move the schedule on its own."""
import numpy as np
import pytest

import oracle
from cpupathtrace_amd import binding, scenes
from tests.util import assert_bits_equal, env

pytestmark = pytest.mark.gpu

SEED = 4242
WORK_STATS = ("rays_traced", "shadow_rays_traced", "node_visits", "leaf_tests", "samples", "vertices")
SCHEDULE_STATS = ("wave_steps", "shading_passes")
CAMERA = scenes.camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0)


def _lit_room():
    """A closed room with Lambertian, glass and mirror objects, an emissive quad and 12 point lights: 14 light samples per path vertex, which
    need the 64-bit slot word."""
    sb = scenes.SceneBuilder()
    sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), sb.material((0.75, 0.7, 0.65, 1.0)))
    sb.sphere((0.35, -0.6, 0.1), 0.35, sb.material((1, 1, 1, 1), 1.5, bsdf=scenes.BSDF_GLASS))
    sb.sphere((-0.45, -0.7, -0.3), 0.28, sb.material((0.9, 0.9, 1.0, 1), bsdf=scenes.BSDF_MIRROR))
    sb.triangles(scenes.make_plane((-0.25, 0.97, -0.25), (0.25, 0.97, 0.25)), sb.material((1, 1, 1, 1), 1.0, (4, 3.5, 3, 1)), cull=True)
    for k in range(12):
        a = 2.0 * np.pi * k / 12
        sb.point_light((0.7 * np.cos(a), 0.3 + 0.05 * k, 0.7 * np.sin(a)), (0.2 + 0.05 * k, 0.3, 0.5 - 0.02 * k, 1.0))
    return sb.build(), CAMERA


def _scene(name):
    if name == "box":  # 14 triangles: tree and triangles in LDS
        return scenes.box_scene()
    if name == "dragonbox":  # 3120 glass triangles in the box: tree in HBM
        return scenes.dragon_box_scene(*scenes.bumpy_sphere_mesh(40, 40, scenes.DRAGON_BOX_TRANSFORM))
    if name == "lit_room":
        return _lit_room()
    if name == "cornell":
        return scenes.cornell_scene(64, 64)
    raise KeyError(name)


def _render(desc, cam, opt, **knobs):
    with env(**knobs):
        scene = binding.Scene(desc)
        try:
            img, st = scene.process_job(cam, opt, base_seed=SEED, want_stats=True)
        finally:
            scene.close()
    return img.copy(), st


@pytest.fixture(scope="module")
def plain():
    """(scene, cam, frame, stats) of a scene at a size and sample count under default settings: rendered once, shared by the cases."""
    cache = {}

    def get(name, w, h, spp):
        key = (name, w, h, spp)
        if key not in cache:
            desc, cam = _scene(name)
            img, st = _render(desc, cam, scenes.options(w, h, spp, spp))
            img.setflags(write=False)
            cache[key] = (desc, cam, img, st)
        return cache[key]

    return get


def _against_oracle(oracle_lib, desc, cam, opt, img, step):
    """Every `step`-th pixel of every `step`-th row (64 pixels at most) through the CPU oracle."""
    w, h = opt["image_width"], opt["image_height"]
    ys, xs = np.mgrid[0:h:step, 0:w:step]
    xs, ys = xs.ravel().astype(np.int32), ys.ravel().astype(np.int32)
    assert 0 < len(xs) <= 64
    states = np.array([binding.seed_to_state(binding.pixel_seed(SEED, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
    handle = oracle_lib.scene_create(desc)
    try:
        want, _ = handle.render_streams(cam, opt, oracle.pixel_streams(xs, ys, states), n_threads=8)
    finally:
        handle.close()
    assert_bits_equal(img[ys, xs], want[ys, xs], "sampled pixels against the oracle")


# scene, width, height, spp, the setting, what is set with it to place the streams (see the module's docstring), step of the oracle's pixel grid (0 = none)
CASES = [
    # a refill after every step for a single idle lane: fewer queued rays than idle lanes, ranks beyond `take`, holes left by cancelled bounces
    ("box", 64, 64, 4, {"PT_BURST": 1, "PT_REFILL_IDLE": 1}, {}, 8),
    # a short ring that fills and wraps every pass or two; the window reload across the wrap
    ("dragonbox", 96, 96, 8, {"PT_ROWS": 1, "PT_SPREAD_WAVES": 16}, {}, 12),
    # refills that wait for nearly empty wavefronts
    ("dragonbox", 96, 96, 8, {"PT_BURST": 3, "PT_REFILL_IDLE": 60}, {}, 0),
    # the wide slot word
    ("lit_room", 32, 32, 4, {"PT_BURST": 1}, {"PT_SPREAD_WAVES": 16}, 4),
    # the small-window instantiation
    ("cornell", 64, 64, 4, {"PT_STACK_WINDOW": 4, "PT_BURST": 1}, {}, 8),
]


def _ids(v):
    return ",".join("%s=%s" % (k[3:].lower(), x) for k, x in v.items()) if isinstance(v, dict) else None


def _same_work(st0, st1, what):
    for k in WORK_STATS:
        assert st1[k] == st0[k], (what, k, st0[k], st1[k])


def _moved(st0, st1):
    return any(st1[k] != st0[k] for k in SCHEDULE_STATS)


@pytest.mark.parametrize("name,w,h,spp,knobs,placement,oracle_step", CASES, ids=_ids)
def test_hand_out_under_odd_settings(plain, oracle_lib, name, w, h, spp, knobs, placement, oracle_step):
    desc, cam, want, st0 = plain(name, w, h, spp)
    opt = scenes.options(w, h, spp, spp)
    if placement:
        placed, st_placed = _render(desc, cam, opt, **placement)
        print("%s %s: %s" % (name, placement, {k: st_placed[k] for k in WORK_STATS + SCHEDULE_STATS}))
        assert_bits_equal(placed, want, "%s: frame under %s" % (name, placement))
        _same_work(st0, st_placed, (name, placement))
        assert _moved(st0, st_placed), "%s: %s changed neither wave_steps nor shading_passes (%s)" % (name, placement, st_placed)
        knobs = dict(placement, **knobs)
    got, st1 = _render(desc, cam, opt, **knobs)
    if placement:
        assert _moved(st_placed, st1), "%s: %s changed neither wave_steps nor shading_passes against %s alone (%s)" % (name, knobs, placement, st1)
    print("%s %s: default %s | set %s" % (name, knobs, {k: st0[k] for k in WORK_STATS + SCHEDULE_STATS}, {k: st1[k] for k in WORK_STATS + SCHEDULE_STATS}))
    assert_bits_equal(got, want, "%s: frame under %s" % (name, knobs))
    _same_work(st0, st1, (name, knobs))
    assert st0["samples"] == w * h * spp and st0["rays_traced"] > st0["shadow_rays_traced"] > 0
    assert _moved(st0, st1), "%s: %s changed neither wave_steps nor shading_passes (%s)" % (name, knobs, st1)
    if oracle_step:
        _against_oracle(oracle_lib, desc, cam, opt, got, oracle_step)


def test_fewer_slots_than_lanes(plain, oracle_lib):
    """8 x 8 pixels: a wavefront uses fewer slots than it has lanes, its ring never holds 64 rays, and every hand-out serves fewer rays
    than there are idle lanes.  At default settings (one slot in each of 64 wavefronts) all 64 pixels against the oracle; the same frame
    and the same work with 16 slots in each of 4 wavefronts, and there again under a refill after every step -- each of which must show in
    the scheduling statistics."""
    desc, cam, want, st0 = plain("dragonbox", 8, 8, 8)
    opt = scenes.options(8, 8, 8, 8)
    assert st0["samples"] == 8 * 8 * 8 and st0["wavefronts"] == 64
    _against_oracle(oracle_lib, desc, cam, opt, want, 1)
    placement = {"PT_SPREAD_WAVES": 4}
    placed, st_placed = _render(desc, cam, opt, **placement)
    knobs = dict(placement, PT_BURST=1, PT_REFILL_IDLE=1)
    got, st1 = _render(desc, cam, opt, **knobs)
    for what, st in (("default", st0), (placement, st_placed), (knobs, st1)):
        print("dragonbox 8x8 %s: %s" % (what, {k: st[k] for k in WORK_STATS + SCHEDULE_STATS}))
    assert st_placed["wavefronts"] == 4
    assert_bits_equal(placed, want, "frame under %s" % placement)
    assert_bits_equal(got, want, "frame under %s" % knobs)
    _same_work(st0, st_placed, placement)
    _same_work(st0, st1, knobs)
    assert _moved(st0, st_placed), "%s changed neither wave_steps nor shading_passes (%s)" % (placement, st_placed)
    assert _moved(st_placed, st1), "%s changed neither wave_steps nor shading_passes against %s alone (%s)" % (knobs, placement, st1)
