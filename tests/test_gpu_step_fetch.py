"""Where a traversal step requests records (Tracer::step), on the GPU.  The rare half of the step (leaves, pops) requests
none any more and none is requested ahead of it: with the tree in LDS every step requests once, at its end, for the lanes that either half
has moved (a scalar lane mask); with the tree in HBM a step that the rare half follows requests once, behind it, for every lane with a
walk, and a step that it does not follow still requests in node_step.  A lane that was moved
and not served -- or served twice, or served with the record of where it stood before -- walks another tree than the reference's, so
every case is 64 x 64 pixels x 16 samples against the C oracle: frame and engine states bit for bit, and the kernel's traversal counters
against the oracle's.

Scenes (each in two forms, see below):
  lds      about 200 triangles, tree and triangles staged in LDS (PT_LDS_SMALL_BYTES raised for the case: the default limit holds about 120; that the library
           staged it is read from what it reports under PT_DEBUG=1);
  hbm      19 800 glass triangles in the box: the tree is read from HBM, the instantiation the benchmark frame runs;
  chain    600 nested triangles with ONE low corner and growing extents, the input that makes the reference's builder split as unevenly as
           it can (a third / two thirds at every node: tests/test_oracle_golden.py): a tree of 13 levels or more whose boxes all overlap at
           that corner, so a walk parks a node at every level, its stack leaves the 8-entry window, and node_step's deep-stack reload runs
           ahead of the step's request;
  flat     a room with flat axis-aligned emitters (ceiling, wall) and an emissive sphere, and a wall of axis-aligned quads at ONE depth whose
           boxes share their coordinates: many equal entry distances, pops that fail the distance test, and walks that node_step sends
           popping in the very step whose pop loop serves them.

Forms.  The kernel does not do all the work of the oracle's shadow rays: it traces none where the result cannot depend on it, and a shadow
walk ends at its first occluder, where the reference finishes a closest-hit query (tests/test_gpu_parity.py:
test_kernel_work_counters_vs_oracle).  With emitters, node_visits, leaf_tests and rays_traced are therefore bounded by the oracle's
counters, by design, and EQUAL them only where no shadow ray exists (test_kernel_work_counters_exact_without_lights).  So every scene is
rendered
  lit      as described: frame and engine states against the oracle, extension rays equal, the other counters bounded by the oracle's;
  dark     the same geometry with the emission taken away, hence without shadow rays: frame and engine states again, and rays_traced,
           node_visits and leaf_tests EQUAL to the oracle's scene queries, slab tests and leaf tests.
Both forms, all four scenes, at PT_LEAF_MIN 1 (the rare step runs in every step, for a single lane, right behind the common half), 8 and
64 (it runs only when no lane stands on an inner node any more).  The environment is held for scene creation AND the render (the knob is
read per job), with PT_SPREAD_WAVES=16: a job is only spread thinner than one row of 64 slots per wavefront up to that many wavefronts, so
the 4096 streams go to 64 wavefronts with a full row and 64 busy lanes each -- spread over the default 1024 wavefronts (4 slots each) no
wavefront ever has 8 lanes waiting, and 8 and 64 would be one schedule.  That each setting took effect
shows in wave_steps, which must differ between any two of them while every work counter stays what it was."""
import contextlib
import os
import sys
import tempfile

import numpy as np
import pytest

import oracle
from cpupathtrace_amd import binding, scenes
from tests.util import assert_bits_equal, env

SEED = 97531
W = H = 64
SPP = 16
LEAF_MINS = (1, 8, 64)
SCENES = ("lds", "hbm", "chain", "flat")
FORMS = ("lit", "dark")
WORK_STATS = ("samples", "vertices", "rays_traced", "shadow_rays_traced", "node_visits", "leaf_tests")
CAMERA = scenes.camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0)
LDS_BYTES = 32768  # records staged in LDS for the `lds` scene
HELD = {"lds": {"PT_LDS_SMALL_BYTES": LDS_BYTES}}


def _emission(lit, rgb):
    return tuple(rgb) + (1,) if lit else (0, 0, 0, 0)


def _lds_scene(lit):
    rng = np.random.default_rng(21)
    sb = scenes.SceneBuilder()
    sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), sb.material((0.75, 0.7, 0.65, 1.0)))
    sb.triangles(scenes.make_plane((-0.3, 0.97, -0.3), (0.3, 0.97, 0.3)), sb.material((1, 1, 1, 1), 1.0, _emission(lit, (4, 3.5, 3))), cull=True)
    mats = [sb.material((0.9, 0.4, 0.3, 1.0)), sb.material((0.3, 0.8, 0.4, 1.0)), sb.material((1, 1, 1, 1), 1.5, bsdf=scenes.BSDF_GLASS),
            sb.material((0.9, 0.9, 1.0, 1.0), bsdf=scenes.BSDF_MIRROR)]
    tri = (rng.uniform(-0.8, 0.8, (184, 1, 3)) + rng.uniform(-0.15, 0.15, (184, 3, 3))).astype(np.float32)
    for k, m in enumerate(mats):
        sb.triangles(tri[k::4], m)
    return sb.build(), CAMERA


def _hbm_scene(lit):
    desc, cam = scenes.dragon_box_scene(*scenes.bumpy_sphere_mesh(100, 100, scenes.DRAGON_BOX_TRANSFORM))
    if not lit:
        materials = desc["materials"].copy()
        materials["emission"] = 0
        desc = dict(desc, materials=materials)
    return desc, cam


def _chain_scene(lit):
    n = 600
    k = np.arange(n, dtype=np.float64)
    s = 0.15 + 1.8 * (k + 1.0) / n           # growing extents from ONE low corner
    z = 0.0015 * k                            # (not coplanar: the far corners step back, the low corner of every box stays (-1, -1, 0))
    tri = np.zeros((n, 3, 3), np.float64)
    tri[:, :, 0] = -1.0
    tri[:, :, 1] = -1.0
    tri[:, 2, 0] += s                         # clockwise seen from +z: the faces look at the camera
    tri[:, 1, 1] += s
    tri[:, 1, 2] = z
    tri[:, 2, 2] = z
    tri = tri.astype(np.float32)
    sb = scenes.SceneBuilder()
    for c in range(4):
        sb.triangles(tri[c::4], sb.material((0.35 + 0.15 * c, 0.9 - 0.15 * c, 0.3 + 0.1 * c, 1.0)))
    # a wall behind, facing the camera like the chain (clockwise seen from +z): every camera ray hits something
    sb.triangles([[(-2, -2, 1.5), (-2, 2, 1.5), (2, 2, 1.5)], [(2, 2, 1.5), (2, -2, 1.5), (-2, -2, 1.5)]], sb.material((0.7, 0.7, 0.75, 1.0)))
    sb.triangles(scenes.make_plane((-1.5, -1.5, -3.5), (1.5, 1.5, -3.5)), sb.material((1, 1, 1, 1), 1.0, _emission(lit, (4, 3.5, 3))))
    return sb.build(), CAMERA


def _flat_scene(lit):
    sb = scenes.SceneBuilder()
    sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), sb.material((0.8, 0.8, 0.8, 1.0)))
    sb.triangles(scenes.make_plane((-0.5, 0.95, -0.5), (0.5, 0.95, 0.5)), sb.material((1, 1, 1, 1), 1.0, _emission(lit, (3, 2.5, 2))))
    sb.triangles(scenes.make_plane((-0.95, -0.5, -0.5), (-0.95, 0.5, 0.5)), sb.material((1, 1, 1, 1), 1.0, _emission(lit, (1, 2, 3))))
    sb.sphere((0.6, 0.5, -0.4), 0.12, sb.material((1, 1, 1, 1), 1.0, _emission(lit, (1, 2, 4))))
    mats = [sb.material((0.9, 0.5, 0.3, 1.0)), sb.material((0.4, 0.6, 0.9, 1.0)), sb.material((0.9, 0.9, 1.0, 1.0), bsdf=scenes.BSDF_MIRROR)]
    for j in range(8):       # a wall of 64 axis-aligned quads at ONE depth, edge to edge in rows: equal box coordinates, equal entry distances
        for i in range(8):
            x, y = -0.8 + 0.2 * i, -0.8 + 0.2 * j
            sb.triangles(scenes.make_plane((x, y, 0.5), (x + 0.2, y + 0.15, 0.5)), mats[(i + j) % 3])
    return sb.build(), CAMERA


_MAKE = {"lds": _lds_scene, "hbm": _hbm_scene, "chain": _chain_scene, "flat": _flat_scene}


@contextlib.contextmanager
def _stderr_text():
    """What the process (the native library included) writes to file descriptor 2 inside the block: yields a function that returns the text."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        done = []

        def text():
            if not done:
                tmp.seek(0)
                done.append(tmp.read().decode(errors="replace"))
            return done[0]

        try:
            yield text
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            text()


def _streams():
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.ravel().astype(np.int32), ys.ravel().astype(np.int32)
    states = np.array([binding.seed_to_state(binding.pixel_seed(SEED, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
    return xs, ys, states


@pytest.fixture(scope="module")
def world(oracle_lib):
    """get(scene, form) -> (desc, cam, the oracle's frame, engine states and counters): made once per scene and form, never written to;
    render(scene, form, leaf_min) -> (frame, engine states, stats, info) of the device under that setting, rendered once."""
    xs, ys, states = _streams()
    opt = scenes.options(W, H, SPP, SPP)
    wanted, rendered = {}, {}

    def get(name, form):
        if (name, form) not in wanted:
            desc, cam = _MAKE[name](form == "lit")
            handle = oracle_lib.scene_create(desc)
            try:
                handle.counters_reset()
                img, after = handle.render_streams(cam, opt, oracle.pixel_streams(xs, ys, states), n_threads=8)
                c = handle.counters()
            finally:
                handle.close()
            img.setflags(write=False)
            after.setflags(write=False)
            wanted[(name, form)] = (desc, cam, img, after, c)
        return wanted[(name, form)]

    def render(name, form, leaf_min):
        key = (name, form, leaf_min)
        if key not in rendered:
            desc, cam = get(name, form)[:2]
            # (PT_DEBUG=1: the library reports on stderr which instantiation of the path kernel it set up -- "scene in LDS" / "scene in HBM")
            with env(PT_LEAF_MIN=leaf_min, PT_SPREAD_WAVES=16, PT_DEBUG=1, **HELD.get(name, {})), _stderr_text() as said:
                scene = binding.Scene(desc)
                try:
                    info = scene.info()
                    img, after, st = scene.process_item(cam, opt, binding.pixel_streams(xs, ys, states), want_stats=True)
                finally:
                    scene.close()
            info["records"] = "LDS" if "scene in LDS" in said() else "HBM" if "scene in HBM" in said() else "?"
            rendered[key] = (img, after, st, info)
        return rendered[key]

    return get, render


def _node_visits(c):
    # two slab tests per inner node + the root test of every query (tests/test_gpu_parity.py)
    assert (c["aabb_tests"] - c["scene_queries"]) % 2 == 0
    return (c["aabb_tests"] - c["scene_queries"]) // 2


@pytest.mark.gpu
@pytest.mark.parametrize("leaf_min", LEAF_MINS)
@pytest.mark.parametrize("name", SCENES)
def test_step_fetch_against_oracle(world, name, leaf_min):
    get, render = world
    for form in FORMS:
        _, _, want, want_after, c = get(name, form)
        img, after, st, info = render(name, form, leaf_min)
        what = "%s, %s, PT_LEAF_MIN=%d" % (name, form, leaf_min)
        print(what, info, {k: st[k] for k in WORK_STATS + ("wave_steps", "shading_passes", "wavefronts")}, c)
        assert st["wavefronts"] == W * H // 64, st  # one full row of 64 slots per wavefront
        if name == "lds":
            assert info["records"] == "LDS", info  # the library staged the scene: the IN_LDS instantiation ran
        if name in ("hbm", "chain"):
            assert info["records"] == "HBM", info
        if name == "chain":
            assert info["depth"] >= 13, info  # the 8-entry window plus a few levels
        assert_bits_equal(img, want, "frame: " + what)
        assert_bits_equal(after, want_after, "engine states: " + what)
        assert st["samples"] == c["samples"] == W * H * SPP
        assert st["vertices"] == c["vertices"] > 0
        assert st["rays_traced"] - st["shadow_rays_traced"] == c["scene_queries"] - c["shadow_rays"], what
        if form == "dark":
            assert c["shadow_rays"] == 0 and st["shadow_rays_traced"] == 0, what
            assert st["rays_traced"] == c["scene_queries"], what
            assert st["node_visits"] == _node_visits(c), what
            assert st["leaf_tests"] == c["tri_tests"] + c["sphere_tests"], what
        else:
            assert (want[..., :3] > 0).any(axis=2).mean() > 0.25, what  # (the frame is lit: equal bits mean something)
            assert 0 < st["shadow_rays_traced"] <= c["shadow_rays"], what
            assert st["rays_traced"] <= c["scene_queries"], what
            assert st["node_visits"] <= _node_visits(c), what
            assert st["leaf_tests"] <= c["tri_tests"] + c["sphere_tests"], what


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_leaf_min_took_effect(world, name):
    _, render = world
    for form in FORMS:
        stats = {m: render(name, form, m)[2] for m in LEAF_MINS}
        print(name, form, {m: (st["wave_steps"], st["shading_passes"]) for m, st in stats.items()})
        for m in LEAF_MINS[1:]:
            for k in WORK_STATS:
                assert stats[m][k] == stats[LEAF_MINS[0]][k], (name, form, m, k)
        steps = [stats[m]["wave_steps"] for m in LEAF_MINS]
        assert len(set(steps)) == len(steps), "%s, %s: wave_steps %s under PT_LEAF_MIN %s" % (name, form, steps, LEAF_MINS)


def test_chain_scene_parks_more_than_the_window(oracle_lib):
    """CPU, by the oracle's own counters: the tree of the chain scene is at least 13 levels deep, and the rays towards the shared low corner
    test more than 9 triangles per query, which a walk can only do by entering both children and returning to the parked one over and over."""
    desc, cam = _chain_scene(True)
    obj, _ = oracle_lib.bvh_dump(desc)
    depth, stack = 0, [1]
    for o in obj:  # pre-order: a negative entry is an inner node
        level = stack.pop()
        depth = max(depth, level)
        if o < 0:
            stack += [level + 1, level + 1]
    assert depth >= 13, depth
    opt = scenes.options(32, 32, 2, 2)
    ys, xs = np.mgrid[16:22, 10:16]  # the lower left of the frame, where every box overlaps
    xs, ys = xs.ravel().astype(np.int32), ys.ravel().astype(np.int32)
    states = np.array([binding.seed_to_state(binding.pixel_seed(SEED, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
    handle = oracle_lib.scene_create(desc)
    try:
        handle.counters_reset()
        handle.render_streams(cam, opt, oracle.pixel_streams(xs, ys, states), n_threads=4)
        c = handle.counters()
    finally:
        handle.close()
    print(depth, c)
    assert c["tri_tests"] > 9 * c["scene_queries"], c
