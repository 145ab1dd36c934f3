"""The batched mesh assembler (pt_mesh_batch_kernels.h: the kernels and the launch chain behind pt_scene_pose and pt_mesh_assemble_batch)
run on the CPU: its own source compiled for the host (tests/hip/pose_probe.hip against tests/hip/host_pose), with std::exclusive_scan and
std::stable_sort in place of hipcub's scan and radix sort.  Expected values come from tests/golden/mesh_assembly.npz only (the compiled
reference's io::loadMesh).  No tolerance; NaN compares by NaN-ness."""
import numpy as np
import pytest

from tests import mesh_cases, pose_cases
from tests.util import assert_bits_equal

F = np.float32


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from tests import pose_probe
    return pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("pose") / "libpose_probe_host.so")))


@pytest.fixture(scope="module")
def golden():
    return np.load(pose_cases.GOLDEN)


def _run(probe, golden, batch, limits=(0, 0, 0)):
    counts, pos, nrm = pose_cases.expected(golden, batch)
    room = pose_cases.total_faces(batch)
    whole_p, out_p = mesh_cases.guarded(room)
    whole_n, out_n = mesh_cases.guarded(room)
    total, got_counts, chunks, scans, sorts = probe.assemble(pose_cases.MESH_LIST, pose_cases.instances_of(batch), room, out_p, out_n, limits)
    what = "%s ... %s" % (batch[0], batch[-1])
    assert got_counts.tolist() == counts and total == sum(counts), (what, got_counts.tolist(), counts)
    mesh_cases.assert_guards(whole_p, room, total, what + ": positions written outside the result")
    mesh_cases.assert_guards(whole_n, room, total, what + ": normals written outside the result")
    assert_bits_equal(out_p[:total], pos, what + ": positions vs the reference")
    assert_bits_equal(out_n[:total], nrm, what + ": normals vs the reference")
    return counts, chunks, scans, sorts


def test_the_fixture_holds_what_the_batches_need(golden):
    """Conditions on the golden file's own numbers."""
    count = lambda m, t, s=0: int(golden["count__" + mesh_cases.case_key(m, t, s)])
    assert (count("degenerate", "identity"), count("degenerate", "projective"), count("degenerate", "tiny")) == (600, 421, 0)
    mesh_cases.share_conditions(600)
    mesh_cases.share_conditions(421)
    assert (count("smoothing", "identity"), count("smoothing", "projective")) == (99, 3)
    for name, (v, f) in mesh_cases.MESHES.items():
        assert_bits_equal(golden["vertices__" + name], v, "fixture vertices")
        assert_bits_equal(golden["faces__" + name], f, "fixture faces")
    for name, m in mesh_cases.TRANSFORMS.items():
        assert_bits_equal(golden["matrix__" + name], m, "fixture matrix")
    counts, _, _ = pose_cases.expected(golden, pose_cases.batch_rotating())
    assert pose_cases.has_empty_between_survivors(counts), counts  # an instance that vanishes between two that stay


@pytest.mark.parametrize("transform", pose_cases.TRANSFORM_NAMES)
def test_one_batch_of_18_instances(probe, golden, transform):
    """Empty meshes, 0 / 1 / 63 / 64 / 65 / 257 faces, the degenerate and the smoothing family, flat and smooth side by side, in ONE chain:
    one scan, one sort."""
    counts, chunks, scans, sorts = _run(probe, golden, pose_cases.batch_uniform(transform))
    assert (chunks, scans) == (1, 1) and sorts == (1 if sum(counts) > 0 else 0)


def test_every_instance_under_its_own_transform(probe, golden):
    counts, chunks, scans, sorts = _run(probe, golden, pose_cases.batch_rotating())
    assert (chunks, scans, sorts) == (1, 1, 1)
    assert pose_cases.has_empty_between_survivors(counts)


def test_single_instances_and_flat_only_batches(probe, golden):
    """A batch of one, and batches without a smooth instance (no corner list, no sort)."""
    for entry in (("smoothing", "identity", 1), ("degenerate", "projective", 1), ("empty", "identity", 1), ("faces1", "mirror", 0)):
        _run(probe, golden, [entry])
    flat = [e for e in pose_cases.batch_rotating() if e[2] == 0]
    _, chunks, scans, sorts = _run(probe, golden, flat)
    assert (chunks, scans, sorts) == (1, 1, 0)


@pytest.mark.parametrize("limits", [(0, 0, 3 * 400), (150, 0, 0), (0, 257, 0)])
def test_chunks_give_the_same_triangles(probe, golden, limits):
    """The split the product makes at 2^31 - 1 corners / 2^32 - 1 vertices or faces, here at limits the 18 instances do pass: consecutive
    chunks, each behind the survivors of the one before, an instance larger than the limit alone in its chunk."""
    batch = pose_cases.batch_rotating()
    want, v, f = 1, 0, 0
    for i, (m, _, _) in enumerate(batch):  # the rule, restated: a chunk takes instances while the sums stay within the limits, and one at least
        nv, nf = len(mesh_cases.MESHES[m][0]), len(mesh_cases.MESHES[m][1])
        over = (limits[0] and v + nv > limits[0]) or (limits[1] and f + nf > limits[1]) or (limits[2] and 3 * (f + nf) > limits[2])
        if i > 0 and over:
            want, v, f = want + 1, 0, 0
        v, f = v + nv, f + nf
    assert want >= 3
    _, got, _, _ = _run(probe, golden, batch, limits)
    assert got == want, (got, want)


def test_range_constants_in_one_launch(probe):
    """kb_fill_ranges: empty ranges at the start, in the middle and at the end; nothing before first_tri is written."""
    ranges = [(5, 0, 7, 1), (5, 3, 1, 0), (8, 0, 9, 1), (8, 0, 9, 1), (8, 300, 0xFFFFFFFF, 1), (308, 1, 4, 0), (309, 0, 6, 1)]
    cull, material, obj = probe.fill_ranges(ranges, 5, 304, 11)
    assert (cull[:5] == 0xA5).all() and (material[:5] == 0xA5A5A5A5).all() and (obj[:5] == 0xA5A5A5A5).all()
    want_cull, want_mat = np.zeros(309, np.uint8), np.zeros(309, np.uint32)
    for first, count, mat, c in ranges:
        want_cull[first:first + count], want_mat[first:first + count] = c, mat
    assert (cull[5:] == want_cull[5:]).all() and (material[5:] == want_mat[5:]).all()
    assert obj[5:].tolist() == list(range(11, 11 + 304))
