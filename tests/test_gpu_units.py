"""The device functions of pt_device.h and pt_libm.h, one unit at a time, on the GPU (tests/hip/unit_probe.hip).

(a) The golden unit vectors recorded from the compiled reference (tests/golden/{rng,aabb,triangle,sphere,bsdf,camera}.npz), replayed
    against the device exactly as tests/test_oracle_golden.py replays them against the C oracle.
(b) The edge families of tests/unit_cases.py against the C oracle, which tests/test_unit_cases_cpu.py holds bit-equal to the compiled
    reference on these very arrays.  Outputs and engine states, bit for bit; slab_walk by value outside its NaN cases.
(c) The device code of pt_libm.h against the same header compiled for the host, which tests/test_abi_cpu.py and tests/test_libm_sincos.py
    hold equal to glibc: device = host header = glibc.  Zero mismatches.  The probe's host pass also compares the host compile with the
    running C library on the same inputs, so a change to the header that both compiles share does not pass unseen.
"""
import numpy as np
import pytest

from tests import unit_cases as uc
from tests.cases import CAMERAS, golden
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    from tests import unit_probe
    p = unit_probe.Probe()
    if p.device_count() < 1:
        pytest.fail("no HIP device: the unit probe has no CPU path")
    return p


def _same(got, want, what):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_bits_equal(np.asarray(g), np.asarray(w), "%s[%d]" % (what, i))


# ---- (a) golden replay ---------------------------------------------------------------------------------------------------------

def test_golden_rng(probe, oracle_lib):
    g = golden("rng")
    draws, _ = probe.rng_draws(1234, 4)
    assert [int(x) for x in draws] == [0x7971212C, 0xB96EC625, 0xA43977A8, 0x16B314CA]
    for i, seed in enumerate(g["seeds"]):
        seed = int(seed)
        draws, st = probe.rng_draws(seed, 1024)
        assert_bits_equal(draws, g["draws"][i], "draws")
        assert st == oracle_lib.rng_state_after(seed, 1024)
        u, st = probe.uniform_floats(seed, 0.0, 1.0, 1024)
        assert_bits_equal(u, g["u01"][i], "u01")
        assert st == oracle_lib.rng_state_after(seed, 1024)  # one draw per float
        assert_bits_equal(probe.uniform_floats(seed, -1.0 / 512.0, 1.0 / 512.0, 1024)[0], g["uab"][i], "uab")
        assert probe.rng_draws(seed, 1000)[1] == int(g["state_after_1000"][i])
    for i, p in enumerate(g["bern_p"]):
        flags, st = probe.bernoulli(1234, float(p), 1024)
        assert_bits_equal(flags, g["bern_flags"][i], "bernoulli")
        assert st == int(g["bern_states"][i])


def test_golden_aabb(probe):
    g = golden("aabb")
    assert_bits_equal(probe.aabb_intersect(g["boxes"], g["rays"]), g["t"], "slab")
    assert_bits_equal(probe.aabb_intersect(g["kat_boxes"], g["kat_rays"]), g["kat_t"], "slab kat")
    # the walk's variant: the same values (the fixtures hold no NaN product)
    assert not uc.slab_nan_mask(g["boxes"], g["rays"]).any()
    assert np.array_equal(probe.slab_walk(g["boxes"], g["rays"]), g["t"])
    assert np.array_equal(probe.slab_walk(g["kat_boxes"], g["kat_rays"]), g["kat_t"])


def test_golden_triangle(probe):
    g = golden("triangle")
    assert_bits_equal(probe.tri_intersect(g["tri"], g["cull"], g["rays"]), g["t"], "tri t")
    assert_bits_equal(probe.tri_normal(g["tri"], g["nrm"], g["pos"]), g["normal"], "tri normal")


def test_golden_sphere(probe):
    g = golden("sphere")
    assert_bits_equal(probe.sphere_intersect(g["sph"], g["rays"]), g["t"], "sphere t")


@pytest.mark.parametrize("name,kind,one_way", uc.BSDF_KINDS)
def test_golden_bsdf(probe, name, kind, one_way):
    g = golden("bsdf")
    r, fac, pd, st = probe.bsdf_propagate(kind, one_way, g["rays"], g["pos"], g["nrm"], float(g["epsilon"][0]), g["ior"], g["states"])
    assert_bits_equal(r, g[name + "_ray"], name + " ray")
    assert_bits_equal(fac, g[name + "_factor"], name + " factor")
    assert_bits_equal(pd, g[name + "_pd"], name + " pd")
    assert_bits_equal(st, g[name + "_states"], name + " states")
    for syn in (0, 1):
        rgba, shade, p = probe.bsdf_spectrum(kind, one_way, g["rays"][:, 3:], g["to_dir"], g["nrm"], g["light"], g["diffuse"], g["specular"], syn)
        assert_bits_equal(rgba, g["%s_spec%d_rgba" % (name, syn)], "spectrum")
        assert_bits_equal(shade, g["%s_spec%d_shade" % (name, syn)], "shade")
        assert_bits_equal(p, g["%s_spec%d_p" % (name, syn)], "p")


@pytest.mark.parametrize("cam", sorted(CAMERAS))
def test_golden_camera(probe, cam):
    g = golden("camera")
    for shoot in (probe.camera_shoot, probe.camera_shoot_lane):
        rays, st = shoot(CAMERAS[cam], g["xy"], float(g["pixel"][0]), float(g["pixel"][1]), g["states"])
        assert_bits_equal(rays, g[cam + "_rays"], "rays")
        assert_bits_equal(st, g[cam + "_states"], "states")


# ---- (b) edge families against the oracle ----------------------------------------------------------------------------------------

def test_slab_family(probe, oracle_lib):
    boxes, rays = uc.slab_family(1)
    want = oracle_lib.aabb_intersect(boxes, rays)
    uc.assert_hits_and_misses(want, "slab")
    assert_bits_equal(probe.aabb_intersect(boxes, rays), want, "slab_test")  # NaN cases included: it restates std::min / std::max
    # slab_walk (v_min_f32 / v_max_f32) is documented to differ in the sign of a zero result and for NaN operands: by value, NaN products left out
    mask = uc.slab_nan_mask(boxes, rays)
    uc.assert_slab_walk_exclusion(mask)
    walk = probe.slab_walk(boxes, rays)
    bad = (walk != want) & ~mask
    assert not bad.any(), "slab_walk: %d of %d differ, first at %d: got %r want %r" % (
        bad.sum(), bad.size, np.argmax(bad), walk[np.argmax(bad)], want[np.argmax(bad)])


def test_triangle_family(probe, oracle_lib):
    tri, cull, rays, nrm, pos = uc.triangle_family(2)
    want = oracle_lib.tri_intersect(tri, cull, rays)
    uc.assert_hits_and_misses(want, "triangle")
    assert_bits_equal(probe.tri_intersect(tri, cull, rays), want, "tri_intersect")
    assert_bits_equal(probe.tri_normal(tri, nrm, pos), oracle_lib.tri_normal(tri, nrm, pos), "tri_normal")


def test_sphere_family(probe, oracle_lib):
    sph, rays = uc.sphere_family(3)
    want = oracle_lib.sphere_intersect(sph, rays)
    uc.assert_hits_and_misses(want, "sphere")
    assert_bits_equal(probe.sphere_intersect(sph, rays), want, "sphere_intersect")


@pytest.mark.parametrize("name,kind,one_way", uc.BSDF_KINDS)
def test_bsdf_propagate_family(probe, oracle_lib, name, kind, one_way):
    rays, pos, nrm, ior, states = uc.bsdf_propagate_family(4)
    for epsilon in uc.EPSILONS:
        want = oracle_lib.bsdf_propagate(kind, one_way, rays, pos, nrm, epsilon, ior, states)
        _same(probe.bsdf_propagate(kind, one_way, rays, pos, nrm, epsilon, ior, states), want, "%s eps=%g (ray, factor, pd, state)" % (name, epsilon))


@pytest.mark.parametrize("name,kind,one_way", uc.BSDF_KINDS)
def test_bsdf_spectrum_family(probe, oracle_lib, name, kind, one_way):
    args = uc.bsdf_spectrum_family(5)
    for synthetic in (0, 1):
        want = oracle_lib.bsdf_spectrum(kind, one_way, *args, synthetic)
        _same(probe.bsdf_spectrum(kind, one_way, *args, synthetic), want, "%s synthetic=%d (rgba, shade, p)" % (name, synthetic))


def test_camera_family(probe, oracle_lib):
    xy, states = uc.camera_family(6)
    for name, cam in uc.camera_cases().items():
        for pixel in uc.PIXEL_SIZES:
            want = oracle_lib.camera_shoot(cam, xy, pixel, pixel * 0.75, states)
            _same(probe.camera_shoot(cam, xy, pixel, pixel * 0.75, states), want, "camera_shoot %s pixel=%g" % (name, pixel))
            _same(probe.camera_shoot_lane(cam, xy, pixel, pixel * 0.75, states), want, "camera_shoot_lane %s pixel=%g" % (name, pixel))


def test_engine_family(probe, oracle_lib):
    n = uc.RNG_DRAWS
    for seed in uc.RNG_SEEDS:
        draws, st = probe.rng_draws(seed, n)
        assert_bits_equal(draws, oracle_lib.rng_draws(seed, n), "draws")
        assert st == oracle_lib.rng_state_after(seed, n)
        for a, b in uc.UNIFORM_RANGES:
            u, st = probe.uniform_floats(seed, a, b, n)
            assert_bits_equal(u, oracle_lib.uniform_floats(seed, a, b, n), "uniform(%g, %g) seed %d" % (a, b, seed))
            assert st == oracle_lib.rng_state_after(seed, n)
        for p in uc.BERNOULLI_P:
            flags, st = probe.bernoulli(seed, p, n)
            want, want_st = oracle_lib.bernoulli(seed, p, n)
            assert_bits_equal(flags, want, "bernoulli(%g) seed %d" % (p, seed))
            assert st == want_st


# ---- (c) device libm against the host compile of the same header ---------------------------------------------------------------------

def _no_mismatch(result, what):
    bad, first, bad_libc = result
    assert bad == 0, "%s: %d inputs differ between device and host, first: %s" % (what, bad, [[hex(int(v)) for v in np.atleast_1d(f)] for f in first])
    assert bad_libc == 0, "%s: the header's host compile differs from the C library on %d of these inputs" % (what, bad_libc)


def test_libm_sincos(probe):
    """sinf_glibc, cosf_glibc and both results of sincosf_glibc.  Stride 61 over [0, 7] from bit pattern 0; windows of +-4096 floats around
    0 (both signs), 0x00800000, k * pi/4 for k = 1..8, and the abstop12 thresholds 2^-12 and 0x3f400000."""
    inputs = uc.sincos_inputs(61)
    assert len(inputs) > 17000000
    _no_mismatch(probe.libm_sincos(inputs), "sincos")


def test_libm_acos(probe):
    """acosf_glibc.  Stride 61 over [-1, 1]; windows of +-4096 floats at +-1 (NaN side included), +-0.5, 0 and the 2^-26 threshold."""
    inputs = uc.acos_inputs(61)
    assert len(inputs) > 34000000
    _no_mismatch(probe.libm_acos(inputs), "acos")


def test_libm_pow_sweep(probe):
    """powf_glibc_full.  Stride 251 over every non-negative base (0 and inf included) x the eleven exponents of unit_cases.POW_EXPONENTS."""
    bases = uc.pow_sweep_bases(251)
    assert len(bases) > 8000000 and len(uc.POW_EXPONENTS) == 11
    _no_mismatch(probe.libm_pow(bases, uc.POW_EXPONENTS.view(np.uint32), full=True), "powf_glibc_full sweep")


def test_libm_pow_pairs(probe):
    """powf_glibc_full on the 2 M random bit pairs of test_abi_cpu.py and on the special pairs: negative bases with integer, half-integer and
    huge exponents, +-0 / +-inf / NaN in either argument, results that are subnormal, underflow or overflow."""
    x, y = uc.pow_random_pairs()
    _no_mismatch(probe.libm_pow(x, y, full=True, paired=True), "powf_glibc_full random pairs")
    x, y = uc.pow_special_pairs()
    _no_mismatch(probe.libm_pow(x, y, full=True, paired=True), "powf_glibc_full special pairs")


def test_libm_pow_unit_interval(probe):
    """powf_glibc(x, 0.5 | 1), the path's own powf: stride 61 over [2^-33, 1], and 0."""
    bases = uc.pow_unit_bases(61)
    assert len(bases) > 4000000
    _no_mismatch(probe.libm_pow(bases, np.array([0.5, 1.0], np.float32).view(np.uint32), full=False), "powf_glibc")
