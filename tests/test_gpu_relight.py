"""Relighting a scene in place (include/pt_relight.h, pt_relight.cpp, pt_relight.hip), bit for bit: after pt_scene_relight from look A
to look B the scene must be, through every entry point, the flat pt_scene_create scene of the host loader's triangles with look B
(tests/relight_cases.py) -- info, emitter registry and CDF, tree, hits, the material column read back, pixels at fixed and adaptive
sample counts, features, a view batch, the device's own emitter sampling in both table forms, and the getters.  One case is compared
with the CPU oracle's pixels directly.  No expected value comes from the code under test; no tolerance anywhere; NaN compares by
NaN-ness."""
import ctypes as C

import numpy as np
import pytest

from cpupathtrace_amd import build_host, scenes
from tests import relight_cases as rc
from tests.util import assert_bits_equal, env

pytestmark = pytest.mark.gpu

F = np.float32
PT_ERR_INVALID, PT_ERR_UNSUPPORTED = 1, 4
MODES = ["host", "device"]
CAMERA, CAMERA_2 = rc.CAMERA, rc.CAMERA_2


@pytest.fixture(scope="module")
def host():
    return C.CDLL(build_host.build())


@pytest.fixture(scope="module")
def small(host):
    instances, matrices = rc.small_instances()
    return instances, matrices, rc.loaded(host, instances, matrices)


def _rays(n=2048, seed=5):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([rng.uniform(-0.95, 0.95, (n, 3)), d], axis=1).astype(F)


RAYS = _rays()
PROBE_POS = np.random.default_rng(11).uniform(-0.9, 0.9, (256, 3)).astype(F)
PROBE_STATES = np.random.default_rng(12).integers(1, 1 << 63, 256, dtype=np.uint64) | np.uint64(1)


def _state(g, frames=True, extras=False):
    """What the entry points say about a scene, as arrays: compared between scenes bit for bit."""
    from tests.scene_probe import SceneProbe
    out = {"info": g.info(), "n_objects": g.n_objects}
    out["bvh topology"], out["bvh boxes"] = g.bvh_dump()
    out["emitter order"], out["emitter cdf"] = g.emissive()
    out["hit t"], out["hit object"] = g.get_intersection(RAYS)
    probe = SceneProbe(g)
    out["probe counts"] = np.array([probe.n_emis, probe.n_object_samples, probe.n_lights])
    out["device cdf"] = probe.emis_cdf()
    for form in ([] if probe.n_emis == 0 else [0, 1] if probe.n_emis <= probe.lds_table_max else [0]):  # (no emitters: nothing to draw from)
        for k, a in enumerate(probe.sample_emissive(form, PROBE_POS, PROBE_STATES)):
            out["sample_emissive form %d output %d" % (form, k)] = a
    if frames:
        out["pixels 4 spp"] = g.process_job(CAMERA, scenes.options(64, 64, 4, 4), base_seed=77)
        out["pixels 4..16 spp"] = g.process_job(CAMERA, scenes.options(64, 64, 4, 16), base_seed=78)
    if extras:
        opt = scenes.options(64, 64, 4, 4)
        out["views"] = g.process_views([CAMERA, CAMERA_2], opt, base_seeds=[5, 6])
        out["features"] = g.render_features(CAMERA, opt)
    return out


def _assert_same_state(a, b, what):
    assert a["info"] == b["info"] and a["n_objects"] == b["n_objects"], (what, a["info"], b["info"], a["n_objects"], b["n_objects"])
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for key in a:
        if key not in ("info", "n_objects"):
            assert_bits_equal(a[key], b[key], "%s: %s" % (what, key))


def _assert_equals_flat(g, geometry, look, what, frames=True, extras=False):
    """The relit scene g against the flat scene of `look` over the same geometry (instances, matrices, loaded triangles); returns the flat
    scene's info."""
    from cpupathtrace_amd import binding
    instances, matrices, triangles = geometry
    flat = rc.flat_scene(triangles, instances, look)
    gb = binding.Scene(flat)
    try:
        _assert_same_state(_state(g, frames, extras), _state(gb, frames, extras), what)
        n_mesh = sum(n for n, _, _ in triangles)
        assert g.n_objects == rc.N_DESC_OBJECTS + n_mesh
        for start, length, at in ((0, rc.N_DESC_TRIS, 0), (rc.N_DESC_OBJECTS, n_mesh, rc.N_DESC_TRIS)):
            pos, nrm, cull, mat = g.triangles(start, length)
            assert_bits_equal(mat, flat["tri_material"][at:at + length], what + ": get_triangles material")
            assert_bits_equal(cull, flat["tri_cull"][at:at + length], what + ": get_triangles cull")
            assert_bits_equal(pos, flat["tri_pos"][at:at + length], what + ": get_triangles positions")
        assert_bits_equal(g.materials().view(np.uint8), rc.materials_of(look).view(np.uint8), what + ": pt_scene_get_materials")
        pos, spectrum = g.point_lights()
        assert_bits_equal(pos, rc.lights_of(look)[0], what + ": light positions")
        assert_bits_equal(spectrum, rc.lights_of(look)[1], what + ": light spectra")
        return gb.info()
    finally:
        gb.close()


def _relight(g, before, after):
    """pt_scene_relight from look `before` to `after`: the whole table and all lights, and the instances whose material differs"""
    pairs = [(i, m) for i, (m0, m) in enumerate(zip(before["instance_materials"], after["instance_materials"])) if m0 != m]
    return g.relight(materials=rc.materials_of(after), point_lights=rc.lights_of(after), instance_materials=pairs or None)


# ---- 1. emitter-count transitions -------------------------------------------------------------------------------------------------------------

# (looks, emitters expected after each, n_object_samples expected after each): the condition of every chain, asserted on the flat scene
CHAINS = {
    "lds table 0-1-17-16-0": ([rc.lit([]), rc.lit([0]), rc.lit([0, 1]), rc.lit([1]), rc.lit([])], [0, 1, 17, 16, 0], [0, 1, 3, 3, 0]),
    "object samples 8-9-98-99": ([rc.lit([2]), rc.lit([2, 0]), rc.lit([3]), rc.lit([3, 0])], [8, 9, 98, 99], [2, 3, 3, 4]),
    "slot word 6-7 lights, 16-17 materials": ([rc.lit([2], 6), rc.lit([2], 7), rc.lit([2], 1, extra_materials=10), rc.lit([2], 1, extra_materials=11)], [8] * 4, [2] * 4),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_emitter_count_transitions(small, mode, chain):
    from cpupathtrace_amd import binding
    from tests.scene_probe import SceneProbe
    instances, matrices, _ = small
    looks, emitters, samples = CHAINS[chain]
    if chain.startswith("slot word"):
        assert [len(l["lights"]) + s for l, s in zip(looks, samples)][:2] == [8, 9] and [len(l["materials"]) for l in looks][2:] == [16, 17]
    with env(PT_BUILD=mode):
        g = binding.Scene(rc.mesh_scene(instances, matrices, looks[0]))
    try:
        g.process_job(CAMERA, scenes.options(64, 64, 4, 4), base_seed=3)  # the workspace is sized for the first look
        tree = g.bvh_dump()
        for k in range(1, len(looks)):
            what = "%s, PT_BUILD=%s, look %d" % (chain, mode, k)
            info = _relight(g, looks[k - 1], looks[k])
            flat_info = _assert_equals_flat(g, small, looks[k], what, extras=(k == 1))
            assert flat_info["n_emissive"] == emitters[k], (what, flat_info)
            assert (info.n_emissive, info.n_object_samples, info.registry_rebuilt) == (emitters[k], samples[k], 1), what
            assert SceneProbe(g).n_object_samples == samples[k]
            for got, want in zip(g.bvh_dump(), tree):
                assert_bits_equal(got, want, what + ": the tree is the one from before")
    finally:
        g.close()


# ---- 2. emitter kinds ----------------------------------------------------------------------------------------------------------------------------

GLOW_BALL = dict(diffuse=(0.2, 0.2, 0.9, 1.0), emission=(0.1, 0.2, 0.9, 1.5))


@pytest.mark.parametrize("mode", MODES)
def test_emitter_kinds(small, mode):
    """Culled and unculled triangles, a sphere, the zero-area triangle under a lit material, a material whose power times the tiny
    triangle's area underflows, and an emission with negative alpha."""
    from cpupathtrace_amd import binding
    instances, matrices, _ = small
    dark = rc.lit([])
    kinds = rc.lit([0, 1], quad=rc.LAMP, ball=GLOW_BALL, tiny=rc.FAINT)
    negative = rc.lit([0], quad=rc.NEGATIVE_ALPHA, ball=rc.NEGATIVE_ALPHA, tiny=rc.LAMP)
    # the conditions: FAINT is lit, and its probability on the tiny triangle is 0 in float32
    with np.errstate(all="ignore"):
        power = (F(rc.FAINT["emission"][0]) + F(0) + F(0)) * F(1)
        assert power >= np.finfo(F).tiny and power * F(rc.TINY_AREA) == 0 and instances[0][2] is False and instances[1][2] is True
    with env(PT_BUILD=mode):
        g = binding.Scene(rc.mesh_scene(instances, matrices, dark))
    try:
        info = _relight(g, dark, kinds)
        flat_info = _assert_equals_flat(g, small, kinds, "emitter kinds, PT_BUILD=%s" % mode)
        # quad 2 (not its zero-area neighbour), sphere 1, tiny 0, instances 1 + 16
        assert flat_info["n_emissive"] == info.n_emissive == 2 + 1 + 0 + 1 + 16
        assert info.n_candidates == 3 + 1 + 1 + 1 + 16  # (candidates: every object with a lit material)
        info = _relight(g, kinds, negative)
        flat_info = _assert_equals_flat(g, small, negative, "negative alpha, PT_BUILD=%s" % mode)
        assert flat_info["n_emissive"] == info.n_emissive == 1 + 1  # instance 0 and the tiny triangle under the lamp
    finally:
        g.close()


def _spread_geometry(host):
    """Single triangles over areas 1e-12 .. 1e6 and the base's sphere: with emission over six decades the CDF has steps that round to
    nothing (the "spread" magnitudes of tests/shading_cases.py)."""
    tri = (np.array([[0, 0, 0], [1, 0.1, 0.05], [0.05, 1, -0.1]], F), np.array([[0, 1, 2]], np.int32))
    sizes = [10.0 ** e for e in (-6, -5, -4, -3, -2, -1, 0, 1, 2, 3, -6, 3, -6, -5, 2)]
    instances = [tri + (k % 2 == 0, False) for k in range(len(sizes))]
    matrices = [rc.place(s, 0.05 * k - 0.3, -0.2, 0.1 * (k % 3)) for k, s in enumerate(sizes)]
    return instances, matrices, rc.loaded(host, instances, matrices)


@pytest.mark.parametrize("mode", MODES)
def test_spread_magnitudes(host, mode):
    from cpupathtrace_amd import binding
    geometry = _spread_geometry(host)
    instances, matrices, triangles = geometry
    n = len(instances)
    kept = sum(count for count, _, _ in triangles)
    assert kept >= n - 3  # (the loader may reject the smallest)
    rng = np.random.default_rng(21)
    lamps = [dict(emission=tuple(float(10.0 ** rng.uniform(-3, 3)) * c for c in (1.0, 0.5, 0.25)) + (1.0 if k % 3 else 0.5,)) for k in range(n)]
    dark = rc.look(rc.table(rc.DULL, rc.DULL, rc.MIRROR, rc.DULL, *([rc.DULL] * n)), rc.n_lights(3), [rc.FIRST_FREE + k for k in range(n)])
    spread = rc.look(rc.table(rc.DULL, rc.LAMP, GLOW_BALL, rc.DULL, *lamps), rc.n_lights(3), [rc.FIRST_FREE + k for k in range(n)])
    with env(PT_BUILD=mode):
        g = binding.Scene(rc.mesh_scene(instances, matrices, dark))
    try:
        info = g.relight(materials=rc.materials_of(spread))  # (a table edit alone: no instance changes its index)
        flat_info = _assert_equals_flat(g, geometry, spread, "spread, PT_BUILD=%s" % mode, frames=False)
        assert flat_info["n_emissive"] == info.n_emissive == 2 + 1 + kept and info.triangles_rewritten == 0
        cdf = g.emissive()[1]
        assert np.count_nonzero(np.diff(cdf) == 0) > 0  # the condition: some steps of the CDF round to nothing
    finally:
        g.close()


# ---- 3. the large case: more candidates than one trip of the scan, flags alternating along the order -------------------------------------------

@pytest.fixture(scope="module")
def large(host):
    """The large geometry and, per look, what the flat scene says (made once, shared by both builders' cases)"""
    from cpupathtrace_amd import binding
    instances, matrices = rc.large_instances()
    triangles = rc.loaded(host, instances, matrices)
    opt = scenes.options(64, 64, 4, 4)
    want = {}
    for first_lit in (True, False):
        gb = binding.Scene(rc.flat_scene(triangles, instances, rc.large_look(first_lit)))
        try:
            want[first_lit] = (gb.emissive(), gb.info(), gb.process_job(CAMERA, opt, base_seed=9))
        finally:
            gb.close()
    return instances, matrices, triangles, want


@pytest.mark.parametrize("mode", MODES)
def test_large_alternating_registry(large, mode):
    """Two interpenetrating grids of about 70,000 triangles, one lit (tests/test_relight_cpu.py asserts the shares on the oracle's order);
    then the other one.  Object list and CDF in full.  PT_BUILD=host walks the host tree's uploaded order, device the builder's own."""
    from cpupathtrace_amd import binding
    from tests.scene_probe import SceneProbe
    instances, matrices, triangles, want = large
    dark = rc.look(rc.large_look()["materials"], rc.n_lights(1), [rc.OFF, rc.OFF])
    with env(PT_BUILD=mode):
        g = binding.Scene(rc.mesh_scene(instances, matrices, dark))
    try:
        assert SceneProbe(g).device_built == (1 if mode == "device" else 0)
        for first_lit in (True, False):
            look = rc.large_look(first_lit)
            info = g.relight(instance_materials=list(enumerate(look["instance_materials"])))
            (want_obj, want_cdf), want_info, want_pixels = want[first_lit]
            got_obj, got_cdf = g.emissive()
            assert len(want_obj) == triangles[0 if first_lit else 1][0] == info.n_emissive == info.n_candidates
            assert_bits_equal(got_obj, want_obj, "large case, PT_BUILD=%s: emitter order" % mode)
            assert_bits_equal(got_cdf, want_cdf, "large case, PT_BUILD=%s: CDF" % mode)
            assert g.info() == want_info
            assert_bits_equal(g.process_job(CAMERA, scenes.options(64, 64, 4, 4), base_seed=9), want_pixels, "large case, PT_BUILD=%s: pixels" % mode)
    finally:
        g.close()


# ---- 4. instance material edits ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_instance_material_edits(small, mode):
    from cpupathtrace_amd import binding
    instances, matrices, triangles = small
    start = rc.lit([0])
    with env(PT_BUILD=mode):
        g = binding.Scene(rc.mesh_scene(instances, matrices, start))
    try:
        first, count = g.instance_ranges()
        assert count.tolist() == rc.SMALL_COUNTS

        def neighbours(i):
            return [g.triangles(int(first[j]), int(count[j])) for j in range(4) if j != i] + [g.triangles(0, rc.N_DESC_TRIS)]

        current = start
        edits = [("one of the instances", [(1, rc.ON)], 1), ("a repeated index", [(2, rc.ON), (2, rc.OFF), (2, rc.ON)], 2),
                 ("to no material", [(1, rc.NO_MATERIAL)], 1), ("from no material", [(1, rc.OFF)], 1)]
        for name, pairs, i in edits:
            before = neighbours(i)
            info = g.relight(instance_materials=pairs)
            after = dict(current, instance_materials=list(current["instance_materials"]))
            for k, m in pairs:
                after["instance_materials"][k] = m
            assert info.triangles_rewritten == rc.SMALL_COUNTS[i] and info.registry_rebuilt == 1, name
            _assert_equals_flat(g, small, after, "%s, PT_BUILD=%s" % (name, mode))
            for got, want in zip(neighbours(i), before):
                for a, b in zip(got, want):
                    assert_bits_equal(a, b, name + ": a neighbouring instance's triangles")
            current = after
    finally:
        g.close()


# ---- 5. the short cut ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_short_cut_keeps_the_registry(small, mode):
    from cpupathtrace_amd import binding
    instances, matrices, _ = small
    a = rc.lit([0, 2], quad=rc.LAMP)
    recoloured = dict(a, materials=[dict(m) for m in a["materials"]])
    recoloured["materials"][rc.WALL] = dict(diffuse=(0.2, 0.9, 0.3, 1.0))
    recoloured["materials"][rc.QUAD] = dict(rc.LAMP, diffuse=(0.5, 0.5, 0.5, 1.0))  # (the emission stays bit-equal)
    moved = dict(recoloured, lights=[((0.3, 0.2, -0.5), (0.9, 0.8, 0.7, 1.0))])
    with env(PT_BUILD=mode):
        g = binding.Scene(rc.mesh_scene(instances, matrices, a))
    try:
        info = g.relight(materials=rc.materials_of(recoloured))
        assert (info.registry_rebuilt, info.triangles_rewritten, info.n_emissive) == (0, 0, 2 + 1 + 8)
        _assert_equals_flat(g, small, recoloured, "a colour, PT_BUILD=%s" % mode)
        info = g.relight(point_lights=rc.lights_of(moved))
        assert info.registry_rebuilt == 0
        _assert_equals_flat(g, small, moved, "a light moved, PT_BUILD=%s" % mode)
        info = g.relight(instance_materials=[(0, rc.ON), (2, rc.ON)])  # (what they have already: nothing changes)
        assert (info.registry_rebuilt, info.triangles_rewritten) == (0, 0)
        info = g.relight(point_lights=rc.lights_of(rc.lit([], 2)))  # (another number of lights is no short cut)
        assert info.registry_rebuilt == 1
        _assert_equals_flat(g, small, dict(moved, lights=rc.lit([], 2)["lights"]), "two lights, PT_BUILD=%s" % mode)
    finally:
        g.close()


# ---- 6. composition with pose, there and back, frames ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_relight_composes_with_pose(host, small, mode):
    """PT_BUILD is held across the poses (a pose reads it anew): under `device` every pose hands the builder's own leaf order over to the
    scene and the next relight walks it; under `host` the order is dropped with the old tree and uploaded again."""
    from cpupathtrace_amd import binding
    from tests.scene_probe import SceneProbe
    instances, matrices, triangles = small
    moved_matrices = [rc.place(0.25, 0.5, 0.2, -0.3, 0.2), rc.place(0.3, -0.3, 0.4, 0.1), rc.place(0.3, 0.2, -0.5, 0.3, 0.5), rc.place(0.3, -0.2, 0.0, -0.4, -0.2)]
    moved = (instances, moved_matrices, rc.loaded(host, instances, moved_matrices))
    a, b = rc.lit([0], quad=rc.LAMP), rc.lit([1, 3], 3, ball=GLOW_BALL)
    opt = scenes.options(64, 64, 4, 8)
    built = 1 if mode == "device" else 0
    with env(PT_BUILD=mode):
        g = binding.Scene(rc.mesh_scene(instances, matrices, a))
        try:
            first = g.process_job(CAMERA, opt, base_seed=77)
            _relight(g, a, b)
            g.pose(moved_matrices)
            assert SceneProbe(g).device_built == built
            _assert_equals_flat(g, moved, b, "relight then pose, PT_BUILD=%s" % mode)
            g.pose(matrices)
            _assert_equals_flat(g, small, b, "posed back: the look stays, PT_BUILD=%s" % mode)
            _relight(g, b, a)
            assert_bits_equal(g.process_job(CAMERA, opt, base_seed=77), first, "A -> B -> A: the first frame")
            g.pose(moved_matrices)
            assert SceneProbe(g).device_built == built
            _relight(g, a, b)
            _assert_equals_flat(g, moved, b, "pose then relight, PT_BUILD=%s" % mode, extras=True)
            # a frame created after a relight is the relit scene's
            frame = binding.Frame(g, CAMERA, opt, base_seed=77)
            try:
                image, _, info = frame.render()
                assert info["status"] == 0
                image = image.copy()
            finally:
                frame.close()
            assert_bits_equal(image, g.process_job(CAMERA, opt, base_seed=77), "a frame created after the relight")
        finally:
            g.close()


# ---- 7. refusals with a scene --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_refusals_leave_the_scene_as_it_was(small, mode):
    from cpupathtrace_amd import binding
    instances, matrices, triangles = small
    a = rc.lit([2], quad=rc.LAMP)
    opt = scenes.options(64, 64, 4, 8)
    plain = binding.Scene(rc.flat_scene(triangles, instances, a))
    with env(PT_BUILD=mode):
        g = binding.Scene(rc.mesh_scene(instances, matrices, a))
    try:
        for call in (lambda: plain.relight(materials=rc.materials_of(a)), plain.materials, plain.point_lights):
            with pytest.raises(binding.PtError) as refused:
                call()
            assert refused.value.code == PT_ERR_UNSUPPORTED
        before = g.process_job(CAMERA, opt, base_seed=77)
        state = _state(g, frames=False)
        bad_kind = rc.materials_of(a)
        bad_kind["bsdf"][2] = 7
        invalid = [dict(instance_materials=[(4, rc.ON)]), dict(instance_materials=[(0, rc.ON), (0xFFFFFFFF, rc.ON)]), dict(instance_materials=[(1, len(a["materials"]))]),
                   dict(materials=rc.materials_of(a)[:rc.ON]),      # the instances' indices fall out of the table
                   dict(materials=rc.materials_of(a)[:rc.TINY]),    # ... and the tiny triangle's
                   dict(materials=bad_kind)]

        def unchanged(what):
            """after EACH refusal: what the entry points say, the getters, and the frame the scene rendered before"""
            _assert_same_state(_state(g, frames=False), state, what)
            assert_bits_equal(g.materials().view(np.uint8), rc.materials_of(a).view(np.uint8), what + ": materials")
            assert_bits_equal(g.point_lights()[0], rc.lights_of(a)[0], what + ": lights")
            assert_bits_equal(g.process_job(CAMERA, opt, base_seed=77), before, what + ": the frame")

        for kwargs in invalid:
            with pytest.raises(binding.PtError) as refused:
                g.relight(**kwargs)
            assert refused.value.code == PT_ERR_INVALID, kwargs
            unchanged("after the refused %s" % sorted(kwargs))
        # a null array with a non-zero count (the binding never makes one: the struct by hand)
        pos, spectrum, index = np.zeros((2, 3), F), np.ones((2, 4), F), np.zeros(1, np.uint32)
        nulls = [dict(set_point_lights=1, n_point_lights=2, light_pos=None, light_spectrum=spectrum.ctypes.data),
                 dict(set_point_lights=1, n_point_lights=2, light_pos=pos.ctypes.data, light_spectrum=None),
                 dict(n_instance_materials=1, instances=None, instance_material=index.ctypes.data),
                 dict(n_instance_materials=1, instances=index.ctypes.data, instance_material=None)]
        for fields in nulls:
            raw = binding.Relight(**fields)
            assert binding.load().pt_scene_relight(g._h, C.byref(raw), None) == PT_ERR_INVALID, fields
            assert b"null" in binding.load().pt_last_error()
            unchanged("after the refused null array %s" % sorted(fields))
        # 31 point lights + 4 emitter samples: known only once the registry exists, and the instance's words are put back
        with pytest.raises(binding.PtError) as refused:
            g.relight(point_lights=rc.lights_of(rc.lit([], 31)), instance_materials=[(3, rc.ON)])
        assert refused.value.code == PT_ERR_UNSUPPORTED and "32" in str(refused.value)
        unchanged("after the refused 31 lights")
        first, count = g.instance_ranges()
        assert (g.triangles(int(first[3]), int(count[3]))[3] == rc.OFF).all()  # (the material words written for the registry pass are back)
        g.relight(point_lights=rc.lights_of(rc.lit([], 29)))  # (29 + the 3 samples of 10 emitters fit)
        g.relight(point_lights=rc.lights_of(a))
        _assert_same_state(_state(g, frames=False), state, "after the refusals")
        _assert_equals_flat(g, small, a, "after the refusals", frames=False)
        assert_bits_equal(g.process_job(CAMERA, opt, base_seed=77), before, "frame after the refusals")
        # a live frame
        frame = binding.Frame(g, CAMERA, opt, base_seed=77)
        with pytest.raises(binding.PtError) as refused:
            g.relight(materials=rc.materials_of(rc.lit([])))
        assert refused.value.code == PT_ERR_INVALID and "frame" in str(refused.value)
        image, _, info = frame.render()
        assert info["status"] == 0
        assert_bits_equal(image, before, "the frame of the scene that refused the relight")
        frame.close()
    finally:
        g.close()
        plain.close()


# ---- 8. the oracle's pixels directly -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_relit_scene_against_the_oracle(oracle_lib, small, mode):
    import oracle
    from cpupathtrace_amd import binding
    instances, matrices, triangles = small
    a, b = rc.lit([]), rc.lit([1, 2], 2, quad=rc.LAMP, ball=GLOW_BALL)
    opt = scenes.options(24, 24, 4, 4)
    with env(PT_BUILD=mode):
        g = binding.Scene(rc.mesh_scene(instances, matrices, a))
    handle = oracle_lib.scene_create(rc.flat_scene(triangles, instances, b))
    try:
        _relight(g, a, b)
        ys, xs = np.mgrid[0:24, 0:24]
        xs, ys = xs.ravel().astype(np.int32), ys.ravel().astype(np.int32)
        states = np.array([binding.seed_to_state(binding.pixel_seed(77, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
        want, _ = handle.render_streams(CAMERA, opt, oracle.pixel_streams(xs, ys, states), n_threads=8)
        assert_bits_equal(g.process_job(CAMERA, opt, base_seed=77), want, "relit scene vs the oracle's pixels")
        obj, cdf = handle.emissive()
        assert_bits_equal(g.emissive()[0], obj, "relit scene vs the oracle's registry")
        assert_bits_equal(g.emissive()[1], cdf, "relit scene vs the oracle's CDF")
    finally:
        handle.close()
        g.close()
