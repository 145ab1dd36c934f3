"""The C oracle against the compiled reference on every edge family of tests/unit_cases.py, bit for bit.  CPU only.

This is what entitles tests/test_gpu_units.py to use the oracle as the reference on the GPU machine, where the compiled reference
does not exist (the arrangement of test_bvh_adversarial_builds_match_reference).  The reference build without assertions is used:
the families hold NaN slabs, unnormalised directions and degenerate triangles on purpose, which the reference's asserts reject.
The same test checks what each family must contain: hits and misses in the hit/miss families, NaN products below the cap in the
slab family.  The probe's cross-compile for gfx950 (a few seconds) is checked here too, so a header change that breaks it shows
without a GPU.
"""
import numpy as np
import pytest

import oracle
from tests import unit_cases as uc
from tests.util import assert_bits_equal


@pytest.fixture(scope="module")
def ref_ndebug(ref_lib):
    return oracle.Checker("ref", ndebug=True)


def _same(got, want, what):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_bits_equal(np.asarray(g), np.asarray(w), "%s[%d]" % (what, i))


def test_slab_family(oracle_lib, ref_ndebug):
    boxes, rays = uc.slab_family(1)
    t = ref_ndebug.aabb_intersect(boxes, rays)
    _same(oracle_lib.aabb_intersect(boxes, rays), t, "slab")
    uc.assert_hits_and_misses(t, "slab")
    mask = uc.slab_nan_mask(boxes, rays)
    uc.assert_slab_walk_exclusion(mask)
    assert not np.isnan(t[~mask]).any()  # the mask covers every NaN the slab test can produce
    assert np.isnan(t).any()             # and the family does reach the NaN behaviour of std::min / std::max


def test_triangle_family(oracle_lib, ref_ndebug):
    tri, cull, rays, nrm, pos = uc.triangle_family(2)
    t = ref_ndebug.tri_intersect(tri, cull, rays)
    _same(oracle_lib.tri_intersect(tri, cull, rays), t, "tri t")
    uc.assert_hits_and_misses(t, "triangle")
    for c in (0, 1):  # both cull values hit and miss
        uc.assert_hits_and_misses(t[cull == c], "triangle cull=%d" % c)
    normal = ref_ndebug.tri_normal(tri, nrm, pos)
    _same(oracle_lib.tri_normal(tri, nrm, pos), normal, "tri normal")
    assert np.isfinite(normal).all(axis=1).mean() > 0.5


def test_sphere_family(oracle_lib, ref_ndebug):
    sph, rays = uc.sphere_family(3)
    t = ref_ndebug.sphere_intersect(sph, rays)
    _same(oracle_lib.sphere_intersect(sph, rays), t, "sphere t")
    uc.assert_hits_and_misses(t, "sphere")
    for part in uc._parts(len(t), 5)[1:3]:  # the tangent parts fall on both sides of discriminant = 0
        uc.assert_hits_and_misses(t[part], "tangent rays")


@pytest.mark.parametrize("name,kind,one_way", uc.BSDF_KINDS)
def test_bsdf_propagate_family(oracle_lib, ref_ndebug, name, kind, one_way):
    rays, pos, nrm, ior, states = uc.bsdf_propagate_family(4)
    for epsilon in uc.EPSILONS:
        want = ref_ndebug.bsdf_propagate(kind, one_way, rays, pos, nrm, epsilon, ior, states)
        _same(oracle_lib.bsdf_propagate(kind, one_way, rays, pos, nrm, epsilon, ior, states), want, "%s eps=%g" % (name, epsilon))
    if kind == oracle.BSDF_GLASS:
        critical = slice(uc._parts(len(ior), 6)[4].start, None)
        total = want[2][critical] == 1.0  # pd = 1: total internal reflection (or ior 1)
        assert 0.10 <= total.mean() <= 0.90, total.mean()


@pytest.mark.parametrize("name,kind,one_way", uc.BSDF_KINDS)
def test_bsdf_spectrum_family(oracle_lib, ref_ndebug, name, kind, one_way):
    args = uc.bsdf_spectrum_family(5)
    for synthetic in (0, 1):
        want = ref_ndebug.bsdf_spectrum(kind, one_way, *args, synthetic)
        _same(oracle_lib.bsdf_spectrum(kind, one_way, *args, synthetic), want, "%s synthetic=%d" % (name, synthetic))


def test_camera_family(oracle_lib, ref_ndebug):
    xy, states = uc.camera_family(6)
    for name, cam in uc.camera_cases().items():
        for pixel in uc.PIXEL_SIZES:
            want = ref_ndebug.camera_shoot(cam, xy, pixel, pixel * 0.75, states)
            _same(oracle_lib.camera_shoot(cam, xy, pixel, pixel * 0.75, states), want, "%s pixel=%g" % (name, pixel))


def test_engine_family(oracle_lib, ref_ndebug):
    n = uc.RNG_DRAWS
    reached_b = 0
    for seed in uc.RNG_SEEDS:
        _same(oracle_lib.rng_draws(seed, n), ref_ndebug.rng_draws(seed, n), "draws")
        assert oracle_lib.rng_state_after(seed, n) == ref_ndebug.rng_state_after(seed, n)
        for a, b in uc.UNIFORM_RANGES:
            want = ref_ndebug.uniform_floats(seed, a, b, n)
            _same(oracle_lib.uniform_floats(seed, a, b, n), want, "uniform(%g, %g)" % (a, b))
            reached_b += int((want == np.float32(b)).sum())
        for p in uc.BERNOULLI_P:
            _same(oracle_lib.bernoulli(seed, p, n), ref_ndebug.bernoulli(seed, p, n), "bernoulli(%g)" % p)
    assert reached_b > 0  # uniform_real_distribution does round up to b on the one-ulp range


def test_probe_cross_compiles_for_gfx950(tmp_path):
    """tests/hip/unit_probe.hip builds with the product's flags where there is no GPU (about five seconds)."""
    from tests import unit_probe
    lib = unit_probe.build(force=True, lib=str(tmp_path / "libunit_probe.so"))
    data = open(lib, "rb").read()
    assert b"gfx950" in data and b"ptu_libm_pow" in data
