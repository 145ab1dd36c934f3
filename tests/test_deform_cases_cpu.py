"""The skinning kernel without a GPU: its own source (cpupathtrace_amd/csrc/pt_deform_kernels.h) compiled for the host
(tests/deform_probe.py) against the NumPy restatement of include/pt_deform.h's arithmetic (tests/deform_ref.py), bit for bit, on every
case family of tests/deform_cases.py and in both forms of the bone table; and that arithmetic against the assembler's transform, whose
dot it takes over.  No tolerance anywhere; NaN compares by NaN-ness."""
import numpy as np
import pytest

from tests import deform_cases, deform_ref
from tests.util import assert_bits_equal

F = np.float32


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from tests import deform_probe
    return deform_probe.Probe(deform_probe.build_host(str(tmp_path_factory.mktemp("deform") / "libdeform_probe_host.so")))


def test_the_families_straddle_the_products_lds_budget(probe):
    assert probe.lds_bones == deform_cases.LDS_BONES
    assert deform_cases.LDS_BONES in deform_cases.BONE_COUNTS and deform_cases.LDS_BONES + 1 in deform_cases.BONE_COUNTS
    assert max(deform_cases.BONE_COUNTS) >= 4 * deform_cases.LDS_BONES
    assert 48 * deform_cases.LDS_BONES * 8 <= 160 * 1024  # 8 blocks of 256 threads, a CU's 32 wavefronts, fit its LDS with their tables


@pytest.mark.parametrize("k", deform_cases.INFLUENCES)
def test_host_compiled_kernel_equals_the_reference(probe, k):
    n_cases = 0
    for name, c in deform_cases.all_cases():
        if c["bone"].shape[1] != k:
            continue
        want = deform_ref.skin(c["rest"], c["bone"], c["weight"], c["bones"])
        n_bones = len(c["bones"])
        # the product's choice (LDS up to the budget, the cache beyond), and the other form wherever the count allows both
        assert_bits_equal(probe.skin(c["rest"], c["bone"], c["weight"], c["bones"]), want, name + ": the product's form")
        if n_bones <= deform_cases.LDS_BONES:
            assert_bits_equal(probe.skin(c["rest"], c["bone"], c["weight"], c["bones"], lds_bones=0), want, name + ": the cache form, forced")
            assert_bits_equal(probe.skin(c["rest"], c["bone"], c["weight"], c["bones"], lds_bones=n_bones), want, name + ": LDS, a budget of exactly this table")
            if n_bones > 1:
                assert_bits_equal(probe.skin(c["rest"], c["bone"], c["weight"], c["bones"], lds_bones=n_bones - 1), want, name + ": a budget one bone short")
        n_cases += 1
    assert n_cases == len(deform_cases.VERTEX_COUNTS) * len(deform_cases.BONE_COUNTS) * len(deform_cases.WEIGHT_KINDS)


def test_the_weight_families_are_what_they_say():
    for kind in deform_cases.WEIGHT_KINDS:
        _, w = deform_cases.rig(1000, 7, 4, kind)
        if kind == "zero":
            assert (w == 0).all()
            c = deform_cases.case(257, 4, 7, kind)
            assert (deform_ref.skin(c["rest"], c["bone"], c["weight"], c["bones"]) == 0).all()  # every vertex at the origin
        elif kind == "wild":
            assert (w < 0).any() and (w > 1).any()
        elif kind == "denormal":
            assert (w == deform_cases.DENORMAL).any() and abs(float(w[1].sum()) - 1.0) < 1e-5
        else:
            assert np.allclose(w.sum(axis=1), 1.0, atol=1e-5) and (w >= 0).all()


@pytest.mark.parametrize("k", deform_cases.INFLUENCES)
@pytest.mark.parametrize("cancelling", [True, False])
def test_poisoned_bones(probe, k, cancelling):
    """NaN and infinite bone entries: no influence is skipped, so a ZERO weight on such a bone gives NaN too."""
    for n_bones, lds in ((5, None), (5, 0), (deform_cases.LDS_BONES + 1, None)):
        rest = deform_cases.rest_vertices(257)
        bones = deform_cases.poison(deform_cases.bone_matrices(n_bones), cancelling)
        bone, weight, poisoned = deform_cases.poisoned_rig(257, n_bones, k)
        want = deform_ref.skin(rest, bone, weight, bones)
        assert np.isfinite(want[~poisoned]).all() and not np.isfinite(want[poisoned]).all(axis=1).any()
        zero_weight = poisoned & (weight[:, k - 1] == 0)
        assert zero_weight.sum() >= 32 and np.isnan(want[zero_weight]).any(axis=1).all()
        if cancelling:
            uses_inf = bone[:, k - 1] == deform_cases.INF_BONE
            assert np.isnan(want[uses_inf]).all()  # (every component: such vertices reject all their faces in the assembler)
        else:
            assert np.isinf(want).any()
        assert_bits_equal(probe.skin(rest, bone, weight, bones, lds_bones=lds), want, "poisoned bones, %d bones, budget %s" % (n_bones, lds))


def test_one_bone_of_weight_one_is_the_assemblers_transform(tmp_path_factory):
    """deform_ref with K = 1, weight 1 equals rows 0 .. 2 of kb_transform's product for an affine matrix (w' = 1, and v * (1 / 1) = v):
    kb_transform's own source, compiled for the host, transforms the corners of triangles that all survive."""
    from tests import pose_probe
    assembler = pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("pose") / "libpose_probe_host.so")))
    rest = deform_cases.rest_vertices(3 * 85, seed=9)
    faces = np.arange(3 * 85, dtype=np.int32).reshape(-1, 3)
    for seed in (11, 12):
        rows = deform_cases.bone_matrices(1, seed=seed, scale=0.5, shift=20.0)
        matrix = np.concatenate([rows[0], np.array([[0, 0, 0, 1]], F)], axis=0)
        pos, nrm = np.zeros((85, 9), F), np.zeros((85, 9), F)
        kept, _, _, _, _ = assembler.assemble([(rest, faces)], [(0, matrix, 0)], 85, pos, nrm)
        assert kept == 85
        got = deform_ref.skin(rest, np.zeros((len(rest), 1), np.uint32), np.ones((len(rest), 1), F), rows)
        assert_bits_equal(got, pos.reshape(-1, 3), "K = 1, weight 1 against kb_transform")
