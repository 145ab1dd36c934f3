"""The C oracle against the compiled reference on the edge vectors of tests/slow_step_cases.py, bit for bit.  CPU only.

The device's triangle test is straight-line code: it divides by a zero determinant, multiplies infinities and NaNs on, and selects -1 where
the reference returned early.  tests/test_gpu_slow_step.py compares it with the oracle on these vectors; this test is what entitles it to
(the arrangement of tests/test_unit_cases_cpu.py): the compiled reference stays the yardstick.  The reference build without assertions is used,
as there: the vectors hold unnormalised and zero directions, NaNs and triangles without area on purpose.  Each family is also checked to
contain what its name says, by the stages of the test evaluated in float32 without the early returns (slow_step_cases.stages)."""
import numpy as np
import pytest

import oracle
from tests import slow_step_cases as sc
from tests.util import assert_bits_equal


@pytest.fixture(scope="module")
def ref_ndebug(ref_lib):
    return oracle.Checker("ref", ndebug=True)


@pytest.fixture(scope="module")
def vectors():
    return sc.edge_vectors()


@pytest.mark.parametrize("family", [name for name, _ in sc.FAMILIES])
def test_oracle_equals_reference(oracle_lib, ref_ndebug, vectors, family):
    tri, cull, rays = vectors[family]
    want = ref_ndebug.tri_intersect(tri, cull, rays)
    assert_bits_equal(oracle_lib.tri_intersect(tri, cull, rays), want, "tri_intersect, %s" % family)


def test_families_hold_what_they_say(ref_ndebug, vectors):
    eps = sc.EPS
    # the determinant: exactly zero, exactly +-epsilon, one ulp either side, and the cull flag decides for the negative ones
    tri, cull, rays = vectors["determinant"]
    det, u, v = sc.stages(tri, rays)
    t = ref_ndebug.tri_intersect(tri, cull, rays)
    for value in (0.0, eps, -eps, np.nextafter(eps, np.float32(1)), np.nextafter(eps, np.float32(0)), -np.nextafter(eps, np.float32(1))):
        assert (det == np.float32(value)).any(), value
    assert not np.signbit(det[det == 0]).any()  # (a dot product starts from +0: the determinant is never -0, whatever the direction's sign)
    assert (t[np.abs(det) <= eps] == -1.0).all()
    inside = (u == 0.25) & (v == 0.25)
    assert (t[inside & (det > eps)] > 0).all() and (t[inside & (det < -eps) & (cull == 1)] == -1.0).all()
    assert (t[inside & (det < -eps) & (cull == 0)] < 0).all() and (t[inside & (det < -eps) & (cull == 0)] != -1.0).any()  # a hit behind the origin, reported as computed
    # barycentrics on the predicates: exactly 0, exactly 1, u + v exactly 1 and its neighbours; vertices and edges hit, their outer neighbours miss
    tri, cull, rays = vectors["barycentric"]
    det, u, v = sc.stages(tri, rays)
    t = ref_ndebug.tri_intersect(tri, cull, rays)
    front = (det > 0)
    for uu, vv in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (0.25, 0.75), (0.0, 0.5), (0.5, 0.0)):
        at = front & (u == np.float32(uu)) & (v == np.float32(vv))
        assert at.any() and (t[at] == 1.0).all(), (uu, vv)
    assert (t[front & (u + v > 1)] == -1.0).all() and (front & (u + v > 1) & (u <= 1) & (v <= 1)).any()
    assert (t[front & ((u < 0) | (v < 0))] == -1.0).all() and (front & (u < 0) & (u > -1e-30)).any()
    assert (t[front & (u == 0) & (v >= 0) & (u + v <= 1)] == 1.0).all()  # -0 is not below 0
    # a ray through a shared edge or vertex is answered for both triangles; the family does hit and miss
    tri, cull, rays = vectors["shared_edge"]
    t = ref_ndebug.tri_intersect(tri, cull, rays)
    assert 0.05 < (t >= 0).mean() < 0.95
    # no area: the determinant is zero (or a rounding residue below epsilon) and nothing is hit
    tri, cull, rays = vectors["degenerate"]
    det, _, _ = sc.stages(tri, rays)
    assert (det == 0).mean() > 0.5
    assert (ref_ndebug.tri_intersect(tri, cull, rays)[np.abs(det) <= eps] == -1.0).all()
    # behind the origin, on the triangle, in front of it; zero components and all-zero directions
    tri, cull, rays = vectors["behind_axis"]
    t = ref_ndebug.tri_intersect(tri, cull, rays)
    assert (t > 0).any() and (t == 0).any() and ((t < 0) & (t != -1.0)).any()
    assert ((rays[:, 3:6] == 0).sum(axis=1) == 2).any() and ((rays[:, 3:6] == 0).sum(axis=1) == 3).any()
    # NaN u, NaN v (with u finite), and results that are NaN because no test turned them away
    tri, cull, rays = vectors["nan"]
    det, u, v = sc.stages(tri, rays)
    t = ref_ndebug.tri_intersect(tri, cull, rays)
    ok_det = ~(np.where(cull == 1, det, np.abs(det)) <= eps)  # (a NaN determinant passes as well)
    assert (ok_det & np.isnan(u)).any() and (ok_det & np.isfinite(u) & (u >= 0) & (u <= 1) & np.isnan(v)).any()
    assert np.isnan(det).any() and np.isinf(det).any()
    assert np.isnan(t).any() and (t[ok_det & np.isnan(u) & np.isnan(v)] != -1.0).all()
