"""The blend-shape kernel without a GPU: its own source (cpupathtrace_amd/csrc/pt_morph_kernels.h) compiled for the host
(tests/morph_probe.py) against the NumPy restatement of include/pt_morph.h's arithmetic (tests/morph_ref.py, and tests/deform_ref.py
behind it for the fused skinning), bit for bit, on every case family of tests/morph_cases.py and in both forms of the tables; and the
host transposition of a set (pt_morph_rows.h) against its restatement.  No tolerance anywhere; NaN compares by NaN-ness."""
import numpy as np
import pytest

from tests import deform_cases, deform_ref, morph_cases, morph_ref
from tests.util import assert_bits_equal

F = np.float32


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from tests import morph_probe
    return morph_probe.Probe(morph_probe.build_host(str(tmp_path_factory.mktemp("morph") / "libmorph_probe_host.so")))


@pytest.fixture(scope="module")
def skin_probe(tmp_path_factory):
    from tests import deform_probe
    return deform_probe.Probe(deform_probe.build_host(str(tmp_path_factory.mktemp("deform") / "libdeform_probe_host.so")))


def test_the_families_straddle_the_products_lds_budget(probe):
    assert probe.lds_targets == morph_cases.LDS_TARGETS
    assert morph_cases.LDS_TARGETS in morph_cases.TARGET_COUNTS and morph_cases.LDS_TARGETS + 1 in morph_cases.TARGET_COUNTS
    # 8 blocks of 256 threads, a CU's 32 wavefronts, fit its LDS with their bone tables and weights
    assert (48 * deform_cases.LDS_BONES + 4 * morph_cases.LDS_TARGETS) * 8 <= 160 * 1024
    assert {k for k, _ in morph_cases.SKINS} == {0, 1, 4, 8} and {b for k, b in morph_cases.SKINS if k} == {2, deform_cases.LDS_BONES + 1}


@pytest.mark.parametrize("n_vertices", morph_cases.VERTEX_COUNTS)
def test_host_compiled_kernel_equals_the_reference(probe, n_vertices):
    n_cases = 0
    for name, n, rest, targets in morph_cases.all_sets():
        if n != n_vertices:
            continue
        n_targets = len(targets)
        for kind in morph_cases.WEIGHT_KINDS:
            w = morph_cases.weights(n_targets, kind)
            morphed = morph_ref.morph(rest, targets, w)  # (once per set and weights; the skins below share it)
            for k, n_bones in morph_cases.SKINS:
                what = "%s, %s weights, K=%d, %d bones" % (name, kind, k, n_bones)
                skin = morph_cases.skin(n, k, n_bones)
                want = morphed if skin is None else deform_ref.skin(morphed, *skin)
                # the product's choice (LDS when weights and bones both fit, the cache otherwise), and the other form wherever both fit
                assert_bits_equal(probe.morph(rest, targets, w, skin), want, what + ": the product's form")
                if n_targets <= morph_cases.LDS_TARGETS and n_bones <= deform_cases.LDS_BONES:
                    assert_bits_equal(probe.morph(rest, targets, w, skin, lds_targets=0), want, what + ": the cache form, forced")
                    if kind == "partition":
                        assert_bits_equal(probe.morph(rest, targets, w, skin, lds_targets=n_targets), want, what + ": a budget of exactly these weights")
                        assert_bits_equal(probe.morph(rest, targets, w, skin, lds_targets=n_targets - 1), want, what + ": a budget one weight short")
                        if k > 0:
                            assert_bits_equal(probe.morph(rest, targets, w, skin, lds_bones=n_bones - 1), want, what + ": a bone budget one bone short")
                n_cases += 1
    assert n_cases == len(morph_cases.TARGET_COUNTS) * len(morph_cases.FORMS) * len(morph_cases.WEIGHT_KINDS) * len(morph_cases.SKINS)


def test_the_families_are_what_they_say():
    for n in morph_cases.VERTEX_COUNTS:
        none, every, last = morph_cases.row_vertices(n)
        for t in morph_cases.TARGET_COUNTS:
            row_start, target, _ = morph_ref.rows(n, morph_cases.target_set(n, t, "sparse"))
            length = np.diff(row_start.astype(np.int64))
            assert length[every] == t  # a row of length T ...
            if none is not None:
                assert length[none] == 0 and none + 1 == every  # ... next to one of length 0 ...
            if last is not None:
                assert length[last] == 1 and target[row_start[last]] == t - 1 and last == every + 1  # ... and one that lists only the last target
                assert every // 64 == last // 64 == none // 64  # in one wavefront
            mixed = morph_cases.target_set(n, t, "mixed")
            assert sum(1 for _, d in mixed if len(d) == 0) == 1  # one empty target
            if t >= 3:
                assert any(i is None for i, _ in mixed) and any(i is not None and len(i) > 0 for i, _ in mixed)
            assert all(i is None for i, _ in morph_cases.target_set(n, min(t, 3), "dense"))
    for kind in morph_cases.WEIGHT_KINDS:
        w = morph_cases.weights(2049, kind)
        if kind == "zero":
            assert (w == 0).all()
        elif kind == "wild":
            assert (w < 0).any() and (w > 1).any()
        elif kind == "denormal":
            assert (w == morph_cases.DENORMAL).any()
        else:
            assert abs(float(w.sum()) - 1.0) < 1e-4 and (w >= 0).all()


def test_zero_weights_leave_the_rest_vertices(probe):
    for n in (1, 257):
        rest = deform_cases.rest_vertices(n)
        targets = morph_cases.target_set(n, 3, "dense")
        assert_bits_equal(probe.morph(rest, targets, np.zeros(3, F)), rest, "all weights zero")  # (no component is -0.0 here: x + 0 * d = x)


@pytest.mark.parametrize("skin", [(0, 0), (4, 2), (8, 257)])
def test_poisoned_deltas(probe, skin):
    """NaN and infinite deltas: no listed target is skipped, so a ZERO weight on such a delta gives NaN too."""
    n = 257
    rest = deform_cases.rest_vertices(n)
    targets, poisoned = morph_cases.poisoned_set(n)
    rig = morph_cases.skin(n, *skin)
    for kind, lds in (("partition", None), ("partition", 0), ("zero", None), ("zero", 0)):
        w = morph_cases.weights(len(targets), kind)
        assert (w[[morph_cases.NAN_TARGET, morph_cases.INF_TARGET]] == 0).all() == (kind == "zero")
        morphed = morph_ref.morph(rest, targets, w)
        assert np.isfinite(morphed[~poisoned]).all() and not np.isfinite(morphed[poisoned]).all(axis=1).any()
        if kind == "zero":
            assert np.isnan(morphed[poisoned]).any(axis=1).all()  # 0 * inf and 0 * NaN
            assert_bits_equal(morphed[~poisoned], rest[~poisoned], "healthy vertices under zero weights")
        want = morphed if rig is None else deform_ref.skin(morphed, *rig)
        assert_bits_equal(probe.morph(rest, targets, w, rig, lds_targets=lds), want, "poisoned deltas, %s weights, budget %s, skin %s" % (kind, lds, skin))


def test_signed_zero(probe):
    """-0.0 + 0 * d is +0.0: a rest component of -0.0 changes its sign where a zero-weight target lists the vertex, and nowhere else."""
    rest, targets, w, listed = morph_cases.signed_zero_case()
    want = morph_ref.morph(rest, targets, w)
    assert (want == 0).all() and np.signbit(want[~listed]).all() and not np.signbit(want[listed]).any()
    for lds in (None, 0):
        assert_bits_equal(probe.morph(rest, targets, w, lds_targets=lds), want, "signed zero, budget %s" % lds)


@pytest.mark.parametrize("k,n_bones", [(1, 2), (4, 2), (8, 257)])
def test_an_all_empty_set_in_front_of_the_skin_is_kd_skin(probe, skin_probe, k, n_bones):
    """With every target empty the morphed vertex is the rest vertex, and the fused kernel must give what kd_skin gives -- through the
    existing probe of pt_deform_kernels.h."""
    for n in (1, 257, 1000):
        rest = deform_cases.rest_vertices(n)
        bone, weight, bones = morph_cases.skin(n, k, n_bones)
        want = skin_probe.skin(rest, bone, weight, bones)
        empty = (np.zeros(0, np.uint32), np.zeros((0, 3), F))
        for n_targets in (1, 3):
            for lds in (None, 0):
                got = probe.morph(rest, [empty] * n_targets, morph_cases.weights(n_targets, "wild"), (bone, weight, bones), lds_targets=lds)
                assert_bits_equal(got, want, "%d empty targets, K=%d, %d bones, %d vertices, budget %s" % (n_targets, k, n_bones, n, lds))


def test_the_host_transposition_is_stable(probe):
    """Two targets that list the same vertex stay in target order, whatever their own order of vertices; the rows are those of the
    restatement, entry for entry."""
    targets = [(np.array([1, 4], np.uint32), np.array([[1, 1, 1], [2, 2, 2]], F)), (np.zeros(0, np.uint32), np.zeros((0, 3), F)),
               (np.array([0, 4], np.uint32), np.array([[3, 3, 3], [4, 4, 4]], F)), (None, np.arange(15, dtype=F).reshape(5, 3) + 10),
               (np.array([4], np.uint32), np.array([[5, 5, 5]], F))]
    row_start, target, delta = probe.rows(5, targets)
    assert row_start.tolist() == [0, 2, 4, 5, 6, 10]
    assert target.tolist() == [2, 3, 0, 3, 3, 3, 0, 2, 3, 4]
    assert delta[6:, 0].tolist() == [2.0, 4.0, 22.0, 5.0]
    for name, n, _, case in morph_cases.all_sets():
        if n in (1, 257):
            want = morph_ref.rows(n, case)
            for got, expected, what in zip(probe.rows(n, case), want, ("row starts", "targets", "deltas")):
                assert_bits_equal(got, expected, name + ": " + what)
            for i in range(n):  # ascending targets inside every row
                assert (np.diff(want[1][want[0][i]:want[0][i + 1]].astype(np.int64)) > 0).all()
