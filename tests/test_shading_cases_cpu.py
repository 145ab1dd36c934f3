"""The shading-side unit cases on the CPU (tests/shading_cases.py): what entitles tests/test_gpu_shading_units.py to use the C oracle as the
reference for the per-pixel estimator of pt_shading.h.

The compiled reference's processItem cannot be handed a contribution sequence, so on these sequences the oracle's estimator -- the very
functions its process_item runs, which tests/test_oracle_golden.py and tests/test_oracle_vs_reference.py pin to the compiled reference on
rendered pixels -- is held bit-equal to an independent NumPy restatement of worker.cpp:149-326 (tests/estimator_ref.py).  NaN compares by
NaN-ness, everything else by bits.  The same file checks what the families must contain (the three outcomes at 10 % each, both sides of
the two acceptance thresholds), the overlap property on the restatement's trace, and the bound on closed candidates that
derive_options of pt_api.cpp relies on, by a sweep over every pair of options.

For the scene-bound units (sample_emissive, object_normal) the compiled reference CAN be driven: the oracle's sample_lights and normal are
held bit-equal to it -- the build with assertions -- on the scenes, positions and engine states the GPU test uses.
"""
import numpy as np
import pytest

from tests import estimator_ref as er
from tests import shading_cases as sc
from tests.shading_cases import SCENES, SEED, assert_same_run, light_case, max_candidates
from tests.util import assert_bits_equal


@pytest.fixture(scope="module")
def oracle_runs(oracle_lib):
    """(options, family, oracle's result) for every pair of options; computed once and left unchanged"""
    runs = []
    for mn, mx in sc.OPTION_SETS:
        contrib, collected, names = sc.estimator_family(mn, mx, SEED)
        assert max_candidates() >= er.closed_candidates_bound(mn, mx)
        runs.append(((mn, mx), (contrib, collected, names), oracle_lib.estimator_run(mn, mx, mx, contrib, collected, max_candidates())))
    return runs


@pytest.mark.parametrize("index", range(len(sc.OPTION_SETS)), ids=["%d-%d" % o for o in sc.OPTION_SETS])
def test_oracle_equals_restatement(oracle_runs, index):
    (mn, mx), (contrib, collected, names), want = oracle_runs[index]
    for bound in sc.stop_bounds(mx):
        got = er.run(mn, mx, bound, contrib, collected)
        assert_same_run(got, want, "min %d max %d bound %d" % (mn, mx, bound), max_candidates())
        # wherever the overlap flag is set, the sample is not the last under the bound and the estimator does not accept at it
        sc.assert_overlap_property(mx, bound, got)
        if mx > 2:
            assert got["overlap"].any() and not got["overlap"].all()


def test_outcome_shares(oracle_runs):
    sc.assert_outcome_shares([sc.outcome_classes(mn, mx, out) for (mn, mx), _, out in oracle_runs])
    # (1, 11) closes the five candidates that no other pair of options reaches
    assert max(int(out["est_i"][:, 5].max()) for _, _, out in oracle_runs) == 5


def test_threshold_families_reach_both_sides(oracle_runs):
    """The sequences aimed at `ratio < 0.2F` and `stddev < 1E-4F` pass and fail their first convergence test, and the ulp nudges alone
    decide it in some group (the seven sequences of a group differ in one value by at most 7 ulp)."""
    for family in ("threshold ratio", "threshold stddev"):
        first, flipped = [], 0
        for (mn, mx), (contrib, collected, names), _ in oracle_runs:
            pick = names == family
            got = er.run(mn, mx, mx, contrib[pick], collected[pick])["first_check"]
            first.append(got)
            groups = got.reshape(-1, len(sc.NUDGES))
            flipped += int(((groups == 0).any(axis=1) & (groups == 1).any(axis=1)).sum())
        first = np.concatenate(first)
        assert (first == 1).sum() >= 10 and (first == 0).sum() >= 10, (family, np.bincount(first + 1))
        assert flipped >= 5, (family, flipped)


def test_families_leave_the_rendered_domain(oracle_runs):
    """Non-finite pixel values, overflowed m2 and negative means do occur: the families reach what no render feeds the estimator."""
    value = np.concatenate([out["value"] for _, _, out in oracle_runs])
    m2 = np.concatenate([out["est_f"][:, 8:12] for _, _, out in oracle_runs])
    mean = np.concatenate([out["est_f"][:, 4:8] for _, _, out in oracle_runs])
    assert np.isnan(value).any() and np.isinf(m2).any() and np.isnan(m2).any() and (mean < 0).any()
    assert 0.5 < np.isfinite(value).all(axis=1).mean() < 1.0


def test_closed_candidates_never_exceed_the_table():
    """derive_options (pt_api.cpp) keeps PT_MAX_CANDIDATES closed candidates per pixel.  Every pair 0 <= min, max <= 4096 through the
    formulas of worker.cpp:158-164: a pixel closes a candidate every candidate_batch_count batches and sees max / stats batches."""
    mn, mx = np.meshgrid(np.arange(4097), np.arange(4097), indexing="ij")
    stats = np.minimum(np.maximum(mn // 4, 1), 64)
    batch = np.maximum(np.maximum(mn, mx // 4) // stats, 2)
    batches = mx // stats
    closed = np.where(batches > 0, (batches - 1) // batch, 0)
    assert closed.max() <= max_candidates()
    assert closed.max() == 5 and closed[1, 11] == 5  # not the 4 that max / (4 S) suggests: both divisions truncate
    for mn_, mx_ in sc.OPTION_SETS + [(0, 0), (3, 4096), (4096, 4096), (1000, 17)]:  # the restatement's scalar form of the same formulas
        assert er.closed_candidates_bound(mn_, mx_) == closed[mn_, mx_]


# ---- scenes: light sampling and normals ------------------------------------------------------------------------------------------------

def test_oracle_lights_equal_reference(oracle_lib, ref_lib):
    """Scene::sampleLights of the compiled reference -- the build WITH assertions: none of them fires on these cases, edge-on emitters,
    vertices and overflowing squares included -- on every scene, position and engine state the GPU test uses."""
    for n_emitters, variant in SCENES:
        scene, handle, emissive, cdf, pos, states, _ = light_case(oracle_lib, n_emitters, variant)
        theirs = ref_lib.scene_create(scene)
        what = "%d emitters, %s" % (n_emitters, variant)
        for got, want, name in zip(handle.sample_lights(pos, states), theirs.sample_lights(pos, states), ("count", "pos", "spectrum", "pd", "state")):
            assert_bits_equal(got, want, "%s: %s" % (what, name))


def test_oracle_normals_equal_reference(oracle_lib, ref_lib):
    """Object::getSurfaceNormal of the compiled reference (asserting build) at the positions the GPU test uses."""
    if not hasattr(ref_lib.lib, "ref_scene_normal"):
        # only a prebuilt library on a machine without the reference's sources can be in this state: oracle.build() rebuilds a library
        # whose sources changed wherever they exist
        pytest.skip("oracle/_ref/libptref.so was built before ref_scene_normal existed and cannot be rebuilt here")
    for n_emitters, variant in SCENES:
        scene, handle, _, _, _, _, _ = light_case(oracle_lib, n_emitters, variant)
        theirs = ref_lib.scene_create(scene)
        obj, at = sc.normal_positions(scene, SEED + 3)
        assert_bits_equal(handle.normal(obj, at)[0], theirs.normal(obj, at)[0], "%d emitters, %s: normal" % (n_emitters, variant))


def test_light_cases_hold_what_they_should(oracle_lib):
    """Registered emitters = the scene's emitters (the zero-area one never registers); n_object_samples takes 1, 2, 3 and 4; the CDF ends
    in exactly 1 (so no draw selects index n_emis) and holds steps that round to nothing; valid and skipped draws each make
    up at least 10 % of all draws; engine states that hit a CDF entry exist for every scene."""
    valid = draws = 0
    samples = set()
    flat_steps = 0
    for n_emitters, variant in SCENES:
        scene, handle, emissive, cdf, pos, states, hits = light_case(oracle_lib, n_emitters, variant)
        assert len(emissive) == n_emitters and sorted(emissive) == list(range(n_emitters))
        assert cdf[-1] == np.float32(1.0) and (np.diff(cdf) >= 0).all()
        flat_steps += int((np.diff(cdf) == 0).sum())
        assert hits >= 1
        s = min(2 + int(np.log10(n_emitters + 1)), n_emitters)
        samples.add(s)
        count = handle.sample_lights(pos, states)[0] - len(scene["light_pos"])
        assert (count >= 0).all() and (count <= s).all()
        valid += int(count.sum())
        draws += s * len(pos)
    assert samples == {1, 2, 3, 4}
    assert flat_steps > 0
    assert 0.10 <= valid / draws <= 0.90, valid / draws


def test_state_for_uniform(oracle_lib):
    """The engine's step inverted: the state computed for a float r draws exactly r; the all-ones draw gives the float below 1, never 1."""
    def seed_of(state):  # RandomEngine(seed): state = seed ^ (~seed << 32), base.h:26
        lo = state & 0xFFFFFFFF
        return ((((state >> 32) ^ (~lo & 0xFFFFFFFF)) & 0xFFFFFFFF) << 32) | lo
    for r in (0.5, 0.25, 0.01777289, 0.99999994, 2.0 ** -9, 0.0):
        state = sc.state_for_uniform(r)
        assert state is not None
        assert_bits_equal(oracle_lib.uniform_floats(seed_of(state), 0.0, 1.0, 1), np.array([r], np.float32), "uniform")
    assert sc.state_for_uniform(1.0) is None and sc.state_for_uniform(2.0 ** -40) is None
    ones = ((0xFFFFFFFF << 32) * sc.ENGINE_MULTIPLIER_INVERSE) & 0xFFFFFFFFFFFFFFFF
    assert oracle_lib.uniform_floats(seed_of(ones), 0.0, 1.0, 1)[0] == np.nextafter(np.float32(1.0), np.float32(0.0))


def test_scene_probe_cross_compiles_for_gfx950(tmp_path):
    """tests/hip/scene_probe.hip builds with the product's flags where there is no GPU."""
    from tests import scene_probe
    lib = scene_probe.build(force=True, lib=str(tmp_path / "libscene_probe.so"))
    data = open(lib, "rb").read()
    assert b"gfx950" in data and b"pts_sample_emissive" in data and b"pts_object_normal" in data


def test_unit_probe_cross_compiles_with_the_estimator_entry(tmp_path):
    """tests/hip/unit_probe.hip, now with pt_shading.h, builds for gfx950 where there is no GPU."""
    from tests import unit_probe
    lib = unit_probe.build(force=True, lib=str(tmp_path / "libunit_probe.so"))
    data = open(lib, "rb").read()
    assert b"gfx950" in data and b"ptu_estimator_run" in data
