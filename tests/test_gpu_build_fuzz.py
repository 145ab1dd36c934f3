"""The device build of the scene (pt_build.hip: impl::constructBVH level by level) against the host recursion (pt_bvh.cpp), the CPU
oracle and, where it was built, the compiled reference, on every adversarial case of tests/build_cases.py: the same tree bit for bit
(topology and boxes), the same emitter table, the same closest hits on aimed, axis-parallel and random rays, and -- for every case of
ordinary magnitudes -- the same rendered pixels and engine states as the oracle.  test_oracle_vs_reference.py pins the oracle to the
reference on the same cases."""
import os

import numpy as np
import pytest

from tests import build_cases
from tests.util import assert_bits_equal, env, miss_equal

pytestmark = pytest.mark.gpu

NAMES = list(build_cases.CASES)
SANE = [name for name in NAMES if not build_cases.CASES[name].extreme]


def _scene(name, mode):
    from cpupathtrace_amd import binding
    with env(PT_BUILD=mode, PT_BUILD_THREADS=16):
        return binding.Scene(build_cases.library_desc(name))


def _nan_object_tests(oracle_lib, desc, rays, chunk=32):
    """Rays for which Triangle::getIntersection or Sphere::getIntersection of at least one object gives NaN (oracle primitives)."""
    bad = np.zeros(len(rays), bool)
    kinds = ((desc["tri_pos"], lambda o, r, i: oracle_lib.tri_intersect(o, np.repeat(desc["tri_cull"][i], len(rays)), r)),
             (desc["sph"], lambda o, r, i: oracle_lib.sphere_intersect(o, r)))
    for objs, test in kinds:
        for first in range(0, len(objs), chunk):
            idx = np.arange(first, min(first + chunk, len(objs)))
            t = test(np.repeat(objs[idx], len(rays), axis=0), np.tile(rays, (len(idx), 1)), idx)
            bad |= np.isnan(t.reshape(len(idx), len(rays))).any(axis=0)
    return bad


@pytest.mark.parametrize("name", NAMES)
def test_device_build_fuzz(oracle_lib, name):
    desc, _ = build_cases.make(name)
    dev, host = _scene(name, "device"), _scene(name, "host")
    try:
        (od, bd), (oh, bh) = dev.bvh_dump(), host.bvh_dump()
        assert len(od) == 2 * len(desc["obj_kind"]) - 1
        assert_bits_equal(od, oh, "%s: topology, device build vs host build" % name)
        assert_bits_equal(bd, bh, "%s: boxes, device build vs host build" % name)
        oo, bo = oracle_lib.bvh_dump(desc)
        assert_bits_equal(od, oo, "%s: topology, device build vs oracle" % name)
        assert_bits_equal(bd, bo, "%s: boxes, device build vs oracle" % name)
        info = dev.info()
        assert info == host.info()
        assert info["depth"] == build_cases.tree_depth(od)
        for a, b in zip(dev.emissive(), host.emissive()):
            assert_bits_equal(a, b, "%s: emissive objects / CDF" % name)
        rays = build_cases.rays(name)
        (td, hd), (th, hh) = dev.get_intersection(rays), host.get_intersection(rays)
        assert_bits_equal(td, th, "%s: closest hit t, device build vs host build" % name)
        assert_bits_equal(hd, hh, "%s: closest hit object, device build vs host build" % name)
    finally:
        dev.close()
        host.close()
    handle = oracle_lib.scene_create(desc)
    try:
        to, oo = handle.intersect(rays)
    finally:
        handle.close()
    if build_cases.CASES[name].kind == "huge":
        # Coordinates near 1e38 overflow a triangle's or a sphere's own intersection arithmetic, which then returns NaN; the reference
        # walk passes that NaN on as a distance (and may prefer it to a real hit, scene.cpp:136-142) where the library's walk treats it
        # as a miss.  The walk, not the build, differs there: the tree and the device-vs-host hits are compared above in full, hits
        # against the oracle only on the rays that meet no NaN object test (from 64 objects on, no ray is left).
        keep = ~_nan_object_tests(oracle_lib, desc, rays)
        td, hd, to, oo = td[keep], hd[keep], to[keep], oo[keep]
    miss_equal(td, to, "%s: closest hit, device build vs oracle" % name)
    assert_bits_equal(hd[to >= 0], oo[to >= 0], "%s: object hit, device build vs oracle" % name)


@pytest.mark.parametrize("name", NAMES)
def test_device_build_fuzz_vs_reference(name):
    """The device-built tree against the compiled reference's (oracle/_ref/libptref.so, made by build() where the reference's sources
    are); a test of its own, so that its absence never hides the oracle comparison above."""
    import oracle
    if not os.path.exists(os.path.join(oracle.HERE, "_ref", "libptref.so")):
        pytest.skip("oracle/_ref/libptref.so not built")
    ref = oracle.Checker("ref")
    desc, _ = build_cases.make(name)
    dev = _scene(name, "device")
    try:
        od, bd = dev.bvh_dump()
    finally:
        dev.close()
    orf, brf = ref.bvh_dump(desc)
    assert_bits_equal(od, orf, "%s: topology, device build vs reference" % name)
    assert_bits_equal(bd, brf, "%s: boxes, device build vs reference" % name)


@pytest.mark.parametrize("name", SANE)
def test_device_build_fuzz_render(oracle_lib, name):
    """A small frame through the device-built tree, pixel for pixel and engine state for engine state against the oracle."""
    from cpupathtrace_amd import binding, scenes
    import oracle
    desc, cam = build_cases.make(name)
    w, h, spp = 20, 16, 6
    opt = scenes.options(w, h, spp, spp)
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.ravel().astype(np.int32), ys.ravel().astype(np.int32)
    seed = build_cases.CASES[name].seed
    states = np.array([binding.seed_to_state(binding.pixel_seed(seed, int(x), int(y))) for x, y in zip(xs, ys)], np.uint64)
    scene = _scene(name, "device")
    try:
        img, after = scene.process_item(cam, opt, binding.pixel_streams(xs, ys, states))
    finally:
        scene.close()
    handle = oracle_lib.scene_create(desc)
    try:
        want, want_after = handle.render_streams(cam, opt, oracle.pixel_streams(xs, ys, states), n_threads=8)
    finally:
        handle.close()
    assert_bits_equal(img, want, "%s: frame" % name)
    assert_bits_equal(after, want_after, "%s: engine states" % name)
