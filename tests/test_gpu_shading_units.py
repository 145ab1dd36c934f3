"""The shading side of the path kernel, one unit at a time, on the GPU.

ESTIMATOR.  The per-pixel estimator of pt_shading.h on the GPU, one sequence per thread (tests/hip/unit_probe.hip: ptu_estimator_run), against the
C oracle on the families of tests/shading_cases.py, which tests/test_shading_cases_cpu.py holds bit-equal to an independent restatement of
worker.cpp:149-326 on these very arrays.

Case for case: pixel value, accepted flag, samples consumed, every field of the final PtEstimator and the closed candidates.  NaN compares
by NaN-ness (the x86 and gfx950 default NaNs differ in sign), everything else by bits; zero mismatches, no tolerance.  The flags of
estimator_safe_to_overlap, recorded before every sample, must equal the restatement's and have the property the path kernel relies on: a
flagged sample is not the last one under the bound and the estimator does not accept at it.

SCENE-BOUND UNITS (tests/hip/scene_probe.hip).  sample_emissive and object_normal / tri_shade_normal on the device tables of scenes the
product built -- by the host builder (pt_bvh.cpp) and by the device builder (pt_build.hip), 1 to 100 emitters -- against the oracle's
sample_lights and normal, which tests/test_shading_cases_cpu.py holds bit-equal to the compiled reference on the same scenes, positions
and engine states.  Both table forms of sample_emissive (global memory; LDS where the scene has at most PT_LDS_TABLE_MAX emitters), the
builders' CDF itself, and normals at hit points of the product's own get_intersection as well as at vertices, edges and off-plane points
of every object.  Bit for bit, NaN by NaN-ness.
"""
import numpy as np
import pytest

from tests import estimator_ref as er
from tests import shading_cases as sc
from tests.shading_cases import SCENES, SEED, assert_same_run, light_case
from tests.util import assert_bits_equal, env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    from tests import unit_probe
    p = unit_probe.Probe()
    if p.device_count() < 1:
        pytest.fail("no HIP device: the unit probe has no CPU path")
    return p


def _run(probe, oracle_lib, mn, mx, done={}):
    """Device against oracle for one pair of options (once per session); returns the device's outcome classes."""
    if (mn, mx) in done:
        return done[(mn, mx)]
    contrib, collected, names = sc.estimator_family(mn, mx, SEED)
    cap = probe.max_candidates()
    assert cap >= er.closed_candidates_bound(mn, mx)
    for bound in sc.stop_bounds(mx):
        what = "min %d max %d bound %d" % (mn, mx, bound)
        want = oracle_lib.estimator_run(mn, mx, bound, contrib, collected, cap)
        got = probe.estimator_run(mn, mx, bound, contrib, collected)
        assert_same_run(got, want, what, cap)
        sc.assert_overlap_property(mx, bound, got, what)
        assert_bits_equal(got["overlap"], er.run(mn, mx, bound, contrib, collected)["overlap"], what + " overlap flags")
    done[(mn, mx)] = sc.outcome_classes(mn, mx, got)
    return done[(mn, mx)]


@pytest.mark.parametrize("mn,mx", sc.OPTION_SETS, ids=["%d-%d" % o for o in sc.OPTION_SETS])
def test_estimator_against_oracle(probe, oracle_lib, mn, mx):
    _run(probe, oracle_lib, mn, mx)


def test_outcome_shares_on_the_device(probe, oracle_lib):
    """Over every pair of options, by the device's answers (held equal to the oracle's case for case): accepted before max, a candidate
    mean, no qualifying candidate -- each at least 10 % of the sequences."""
    sc.assert_outcome_shares([_run(probe, oracle_lib, mn, mx) for mn, mx in sc.OPTION_SETS])


# ---- scene-bound units -------------------------------------------------------------------------------------------------------------------

BUILDERS = ["host", "device"]


def _device_scene(scene, builder):
    from cpupathtrace_amd import binding
    from tests import scene_probe
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the scene probe has no CPU path")
    with env(PT_BUILD=builder, PT_BUILD_THREADS=16):
        gpu = binding.Scene(scene)
    probe = scene_probe.SceneProbe(gpu)
    assert probe.device_built == (1 if builder == "device" else 0)
    return gpu, probe


def _run_lights(oracle_lib, n_emitters, variant, builder, done={}):
    """sample_emissive against the oracle for one scene and builder, every form the scene has (once per session); returns (valid draws,
    draws) summed over the forms."""
    key = (n_emitters, variant, builder)
    if key in done:
        return done[key]
    scene, handle, emissive, cdf, pos, states, _ = light_case(oracle_lib, n_emitters, variant)
    gpu, probe = _device_scene(scene, builder)
    try:
        what = "%d emitters, %s, %s build" % key
        assert probe.n_emis == len(emissive) and probe.n_lights == len(scene["light_pos"])
        assert probe.n_object_samples == min(2 + int(np.log10(len(emissive) + 1)), len(emissive))
        assert_bits_equal(probe.emis_cdf(), cdf, what + ": CDF")
        want = handle.sample_lights(pos, states)
        forms = [0, 1] if probe.n_emis <= probe.lds_table_max else [0]
        valid = draws = 0
        for form in forms:
            got = probe.sample_lights(form, pos, states, scene["light_pos"], scene["light_spectrum"])
            for g, w, name in zip(got[:5], want, ("count", "pos", "spectrum", "pd", "state")):
                assert_bits_equal(g, w, "%s, form %d: %s" % (what, form, name))
            valid, draws = valid + int(got[5].sum()), draws + got[5].size
        if forms == [0]:
            from tests.scene_probe import ProbeError
            with pytest.raises(ProbeError):  # the LDS form does not exist beyond PT_LDS_TABLE_MAX emitters
                probe.sample_emissive(1, pos[:1], states[:1])
    finally:
        gpu.close()
    done[key] = (valid, draws)
    return done[key]


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n_emitters,variant", SCENES, ids=["%d-%s" % s for s in SCENES])
def test_sample_emissive_against_oracle(oracle_lib, n_emitters, variant, builder):
    _run_lights(oracle_lib, n_emitters, variant, builder)


def test_light_draw_shares_on_the_device(oracle_lib):
    """Valid and skipped draws each make up at least 10 % of all draws, over every scene and builder, by the device's answers (held equal
    to the oracle's case for case)."""
    counts = [_run_lights(oracle_lib, e, v, b) for e, v in SCENES for b in BUILDERS]
    valid, draws = sum(c[0] for c in counts), sum(c[1] for c in counts)
    assert 0.10 <= valid / draws <= 0.90, valid / draws


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n_emitters,variant", SCENES, ids=["%d-%s" % s for s in SCENES])
def test_object_normal_against_oracle(oracle_lib, n_emitters, variant, builder):
    scene, handle, emissive, _, _, _, _ = light_case(oracle_lib, n_emitters, variant)
    gpu, probe = _device_scene(scene, builder)
    try:
        what = "%d emitters, %s, %s build" % (n_emitters, variant, builder)
        obj, at = sc.normal_positions(scene, SEED + 3)
        # hit points of the product's own traversal: rays from outside towards the emitters' region
        rng = np.random.default_rng([SEED, n_emitters, 4])
        origin = rng.uniform(-4, 12, (256, 3)).astype(np.float32)
        origin[:, 2] = 9.0
        target = rng.uniform(-1, 9, (256, 3)).astype(np.float32)
        target[:, 2] = rng.uniform(-3, 3, 256)
        direction = target - origin
        direction /= np.linalg.norm(direction, axis=1)[:, None].astype(np.float32)
        t, hit = gpu.get_intersection(np.concatenate([origin, direction], axis=1))
        reached = hit >= 0
        assert reached.sum() >= 64, what
        obj = np.concatenate([obj, hit[reached]]).astype(np.int32)
        at = np.concatenate([at, (origin + direction * t[:, None])[reached]]).astype(np.float32)

        want_n, want_material = handle.normal(obj, at)
        lds = probe.n_emis <= probe.lds_table_max
        got = probe.object_normal(obj, at, lds=lds)
        assert_bits_equal(got[0], want_n, what + ": object_normal")
        assert_bits_equal(got[1], want_material, what + ": material index")
        if lds:
            found = got[2].astype(bool)
            is_tri = np.asarray(scene["obj_kind"])[obj] == 0
            assert (found == (is_tri & np.isin(obj, emissive))).all(), what
            assert found.any()
            assert_bits_equal(got[3][found], want_n[found], what + ": tri_shade_normal on the LDS record")
            assert_bits_equal(got[4][found], want_material[found], what + ": material index of the LDS record")
    finally:
        gpu.close()
