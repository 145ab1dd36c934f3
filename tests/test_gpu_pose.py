"""Re-posing mesh instances in place (include/pt_pose.h, pt_pose.cpp, pt_mesh_batch.hip), bit for bit: pt_mesh_assemble_batch against
the golden answers of the compiled reference (tests/golden/mesh_assembly.npz), and a posed scene against a flat pt_scene_create scene of
the triangles the host loader (pth_load_mesh, which tests/test_mesh_cases_cpu.py holds equal to the reference) returns for the new
matrices: info, tree, emitters, hits, triangles read back, pixels, views and features.  No expected value comes from the code under test.
No tolerance anywhere; NaN compares by NaN-ness."""
import ctypes as C

import numpy as np
import pytest

from cpupathtrace_amd import build_host, scenes
from tests import mesh_cases, pose_cases
from tests.util import assert_bits_equal, env

pytestmark = pytest.mark.gpu

F = np.float32
PT_ERR_INVALID, PT_ERR_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def host():
    return C.CDLL(build_host.build())


@pytest.fixture(scope="module")
def golden():
    return np.load(pose_cases.GOLDEN)


# ---- 1. the batched assembler on its own ---------------------------------------------------------------------------------------------------

def _assemble(golden, batch):
    from cpupathtrace_amd import binding
    counts, pos, nrm = pose_cases.expected(golden, batch)
    cap = pose_cases.total_faces(batch) + 3
    whole_p, out_p = mesh_cases.guarded(cap)
    whole_n, out_n = mesh_cases.guarded(cap)
    total, got_counts, got_pos, got_nrm = binding.mesh_assemble_batch(pose_cases.MESH_LIST, pose_cases.instances_of(batch), capacity=cap, out_pos=out_p, out_nrm=out_n)
    what = "%s ... %s" % (batch[0], batch[-1])
    assert got_counts.tolist() == counts and total == sum(counts), (what, got_counts.tolist(), counts)
    mesh_cases.assert_guards(whole_p, cap, total, what + ": positions written outside the result")
    mesh_cases.assert_guards(whole_n, cap, total, what + ": normals written outside the result")
    assert_bits_equal(got_pos, pos, what + ": positions vs the reference")
    assert_bits_equal(got_nrm, nrm, what + ": normals vs the reference")
    return total, pos, nrm


@pytest.mark.parametrize("transform", pose_cases.TRANSFORM_NAMES + ["rotating"])
def test_assemble_batch_matches_golden(golden, transform):
    from cpupathtrace_amd import binding
    batch = pose_cases.batch_rotating() if transform == "rotating" else pose_cases.batch_uniform(transform)
    total, pos, nrm = _assemble(golden, batch)
    if total > 1:
        # a capacity smaller than the result: the counts come back and nothing is written past the capacity
        small = total // 2
        whole_p, out_p = mesh_cases.guarded(small)
        whole_n, out_n = mesh_cases.guarded(small)
        n2, _, pos2, nrm2 = binding.mesh_assemble_batch(pose_cases.MESH_LIST, pose_cases.instances_of(batch), capacity=small, out_pos=out_p, out_nrm=out_n)
        assert n2 == total and len(pos2) == small
        mesh_cases.assert_guards(whole_p, small, small, "positions written past the capacity")
        mesh_cases.assert_guards(whole_n, small, small, "normals written past the capacity")
        assert_bits_equal(pos2, pos[:small], "positions, small capacity")
        assert_bits_equal(nrm2, nrm[:small], "normals, small capacity")
    if transform == "rotating":
        assert pose_cases.has_empty_between_survivors(pose_cases.expected(golden, batch)[0])
        for entry in (("smoothing", "identity", 1), ("degenerate", "projective", 0), ("empty", "identity", 1)):  # batches of one
            _assemble(golden, [entry])


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------

IN_BOX = np.array(scenes.DRAGON_BOX_TRANSFORM, F)  # the bumpy sphere (radius 40 around (0, 50, 0)) into the unit box
SMALL_IN_BOX = np.array([[0.015, 0, 0, 0.1], [0, 0.02, 0, -0.1], [0, 0, 0.015, 0.2], [0, 0, 0, 1]], F)  # the +-40 families
COLLAPSE = np.diag(np.array([0, 0, 0, 1], F))  # every vertex to the origin: every face is rejected
PROJECTIVE = mesh_cases.TRANSFORMS["projective"]
CAMERA = scenes.camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0)
CAMERA_2 = scenes.camera((1.5, 0.5, -2.5), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0)
MATERIALS = dict(glass=dict(diffuse=(1, 1, 1, 1), ior=1.5, bsdf=scenes.BSDF_GLASS), white=dict(diffuse=(0.8, 0.7, 0.6, 1.0)),
                 lamp=dict(diffuse=(1, 1, 1, 1), emission=(1.0, 0.9, 0.8, 2.0)))


def _shift(m, dx, dy, dz, scale=1.0):
    out = np.array(m, F)
    out[:3, :3] *= F(scale)
    out[:3, 3] += np.array([dx, dy, dz], F)
    return out


def _base(sb):
    """The Box's walls and light quad, a sphere and a point light: both object kinds and both light kinds (as tests/test_gpu_mesh.py)."""
    sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)))
    light = sb.material((1, 1, 1, 1), 1.0, (1, 1, 1, 1))
    sb.triangles(scenes.make_plane((-0.25, F(1.0) - F(0.01), -0.25), (0.25, F(1.0) - F(0.01), 0.25)), light)
    sb.sphere((0.55, -0.7, -0.3), 0.3, sb.material((0, 0, 1, 1), bsdf=scenes.BSDF_MIRROR))
    sb.point_light((-0.6, 0.7, -0.6), (0.5, 0.5, 0.4, 1.0))


def _mesh_scene(instances, matrices):
    """The description with the instances (vertices, faces, material name, cull, smooth) under `matrices`, for pt_scene_create_meshes."""
    sb = scenes.SceneBuilder()
    _base(sb)
    mats = {name: sb.material(**kw) for name, kw in MATERIALS.items()}
    mats[None] = scenes.NO_MATERIAL
    for (v, f, material, cull, smooth), m in zip(instances, matrices):
        sb.mesh(v, f, m, mats[material], cull=cull, smooth=smooth)
    return sb.build()


def _flat_scene(host, instances, matrices):
    """(flat description, loader counts): the loader's triangles for the matrices appended in instance order with explicit normals."""
    sb = scenes.SceneBuilder()
    _base(sb)
    mats = {name: sb.material(**kw) for name, kw in MATERIALS.items()}
    mats[None] = scenes.NO_MATERIAL
    counts = []
    for (v, f, material, cull, smooth), m in zip(instances, matrices):
        n, pos, nrm = mesh_cases.load_mesh(host, "pth_", v, f, m, int(smooth))
        counts.append(n)
        if n > 0:
            sb.triangles(pos.reshape(-1, 3, 3), mats[material], cull=cull, normals=nrm.reshape(-1, 3, 3))
    return sb.build(), counts


def _rays(n=4096, seed=5):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([rng.uniform(-0.95, 0.95, (n, 3)), d], axis=1).astype(F)


RAYS = _rays()


def _state(g, spp=(4, 8), frame=True):
    """What the entry points say about a scene, as arrays: compared between scenes bit for bit."""
    out = {"info": g.info(), "n_objects": g.n_objects}
    out["bvh topology"], out["bvh boxes"] = g.bvh_dump()
    out["emitter order"], out["emitter cdf"] = g.emissive()
    out["hit t"], out["hit object"] = g.get_intersection(RAYS)
    if frame:
        out["pixels"] = g.process_job(CAMERA, scenes.options(64, 64, *spp), base_seed=77)
    return out


def _assert_same_state(a, b, what):
    assert a["info"] == b["info"] and a["n_objects"] == b["n_objects"], (what, a["info"], b["info"], a["n_objects"], b["n_objects"])
    for key in a:
        if key not in ("info", "n_objects"):
            assert_bits_equal(a[key], b[key], "%s: %s" % (what, key))


def _assert_posed_equals_flat(host, ga, instances, matrices, what, spp=(4, 8), frame=True, extras=False):
    """Everything tests/test_gpu_mesh.py::_assert_same_scene compares, between the posed scene and a flat scene of the loader's triangles
    at the same matrices; returns the flat scene's info and the loader's counts."""
    from cpupathtrace_amd import binding
    flat, counts = _flat_scene(host, instances, matrices)
    assert_bits_equal(ga.pose_transforms(), np.array(matrices, F).reshape(-1, 4, 4), what + ": pt_scene_get_pose")
    gb = binding.Scene(flat)
    try:
        n_desc = len(flat["obj_kind"]) - sum(counts)
        first, count = ga.instance_ranges()
        assert count.tolist() == counts, (what, count.tolist(), counts)
        assert first.tolist() == (n_desc + np.concatenate([[0], np.cumsum(counts)[:-1]])).astype(np.int64).tolist(), what
        assert ga.n_objects == gb.n_objects == n_desc + sum(counts), what
        _assert_same_state(_state(ga, spp, frame), _state(gb, spp, frame), what)
        n_tri_desc = len(flat["tri_pos"]) - sum(counts)  # (the description's triangles are its first objects, the sphere follows them: _base)
        for start, length, at in ((0, n_tri_desc, 0), (n_desc, sum(counts), n_tri_desc), (n_tri_desc - 2, 2, n_tri_desc - 2)):
            pos, nrm, cull, mat = ga.triangles(start, length)
            assert_bits_equal(pos, flat["tri_pos"][at:at + length], what + ": get_triangles positions")
            assert_bits_equal(nrm, flat["tri_nrm"][at:at + length], what + ": get_triangles normals")
            assert_bits_equal(cull, flat["tri_cull"][at:at + length], what + ": get_triangles cull")
            assert_bits_equal(mat, flat["tri_material"][at:at + length], what + ": get_triangles material")
        if extras:
            opt = scenes.options(64, 64, 4, 4)
            assert_bits_equal(ga.process_views([CAMERA, CAMERA_2], opt, base_seeds=[5, 6]), gb.process_views([CAMERA, CAMERA_2], opt, base_seeds=[5, 6]), what + ": views")
            assert_bits_equal(ga.render_features(CAMERA, opt), gb.render_features(CAMERA, opt), what + ": first-hit features")
            assert_bits_equal(ga.render_features(CAMERA, opt, followed={}), gb.render_features(CAMERA, opt, followed={}), what + ": followed features")
        return gb.info(), counts
    finally:
        gb.close()


def _sphere(nu, nv):
    return scenes.bumpy_sphere_vertices(nu, nv)


def _four_instances():
    v1, f1 = _sphere(24, 16)
    v2, f2 = _sphere(48, 24)
    v3, f3 = mesh_cases.MESHES["faces64"]
    v4, f4 = mesh_cases.MESHES["degenerate"]
    instances = [(v1, f1, "glass", False, True), (v2, f2, "white", True, True), (v3, f3, None, False, False), (v4, f4, "glass", True, True)]
    pose_a = [_shift(IN_BOX, -0.4, -0.3, 0.2, 0.5), _shift(IN_BOX, 0.3, 0.1, 0.3, 0.5), SMALL_IN_BOX, _shift(SMALL_IN_BOX, -0.3, 0.2, -0.4)]
    pose_b = [_shift(IN_BOX, 0.2, 0.3, -0.2, 0.4), _shift(IN_BOX, -0.35, -0.2, 0.1, 0.6), _shift(SMALL_IN_BOX, 0.2, 0.3, 0.1), SMALL_IN_BOX @ PROJECTIVE]
    return instances, pose_a, pose_b


# ---- 2. a posed scene is the fresh flat scene ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["host", "device", None])
def test_posed_scene_equals_flat_scene(host, mode):
    from cpupathtrace_amd import binding
    instances, pose_a, pose_b = _four_instances()
    with env(PT_BUILD=mode) if mode else env():
        g = binding.Scene(_mesh_scene(instances, pose_a))
        try:
            g.process_job(CAMERA, scenes.options(64, 64, 4, 4), base_seed=3)  # the workspace is sized for pose A
            info = g.pose(pose_b)
            assert (info["n_instances"], info["assembly_syncs"], info["assembly_chunks"]) == (4, 1, 1)
            _, counts = _assert_posed_equals_flat(host, g, instances, pose_b, "pose B, PT_BUILD=%s" % mode)
            assert info["n_triangles"] == sum(counts)
        finally:
            g.close()


def test_one_wait_for_a_batch_of_1_and_of_18(host):
    """assembly_syncs and assembly_chunks of a scene with one instance and with the 18 of the assembler's tests (9 meshes x flat / smooth)."""
    from cpupathtrace_amd import binding
    eighteen = [(v, f, None, False, bool(s)) for v, f in pose_cases.MESH_LIST for s in (0, 1)]
    for instances in (eighteen[14:15], eighteen):
        pose_a = [_shift(SMALL_IN_BOX, 0.01 * i, 0, 0) for i in range(len(instances))]
        pose_b = [COLLAPSE if i == 8 else _shift(SMALL_IN_BOX, 0, 0.01 * i, 0.1) for i in range(len(instances))]  # (8 vanishes between two that stay)
        g = binding.Scene(_mesh_scene(instances, pose_a))
        try:
            info = g.pose(pose_b)
            assert (info["n_instances"], info["assembly_syncs"], info["assembly_chunks"]) == (len(instances), 1, 1)
            _, counts = _assert_posed_equals_flat(host, g, instances, pose_b, "%d instances" % len(instances), frame=False)
            assert info["n_triangles"] == sum(counts) and pose_cases.has_empty_between_survivors(counts) == (len(instances) == 18)
        finally:
            g.close()


# ---- 3. the crossing pose: everything the workspace was sized from changes ----------------------------------------------------------------

def test_pose_across_builder_lds_and_emitter_thresholds(host):
    """Pose A collapses both instances to a point (0 triangles): the scene is the base alone -- host builder, tree in LDS, 2 emitters.
    Pose B expands 2208 + 720 emissive triangles: device builder, tree in HBM, deeper, emitters past the LDS table.  A stale spill depth
    or LDS decision would show in the hits, the features and the pixels."""
    from cpupathtrace_amd import binding
    (v1, f1), (v2, f2) = _sphere(48, 24), _sphere(24, 16)
    instances = [(v1, f1, "lamp", False, True), (v2, f2, "lamp", True, False)]
    pose_a = [COLLAPSE, COLLAPSE]
    pose_b = [_shift(IN_BOX, -0.3, -0.2, 0.2, 0.6), _shift(IN_BOX, 0.4, 0.3, -0.1, 0.4)]
    g = binding.Scene(_mesh_scene(instances, pose_a))
    try:
        info_a, counts_a = _assert_posed_equals_flat(host, g, instances, pose_a, "created at A", extras=True)
        g.pose(pose_b)
        info_b, counts_b = _assert_posed_equals_flat(host, g, instances, pose_b, "posed to B", extras=True)
        g.pose(pose_a)
        _assert_posed_equals_flat(host, g, instances, pose_a, "posed back to A", extras=True)
        # the condition, on the reference side: the flat scenes differ in what the workspace is sized from
        assert counts_a == [0, 0] and counts_b == [2208, 720]
        assert info_a["n_emissive"] == 2 and info_b["n_emissive"] == 2 + 2208 + 720 > 16
        assert info_b["depth"] > info_a["depth"] and info_a["n_nodes"] < 2 * 1024 <= info_b["n_nodes"]
    finally:
        g.close()


# ---- 4. ranges move -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["host", "device"])
def test_ranges_behind_a_posed_instance_move(host, mode):
    from cpupathtrace_amd import binding
    v, f = mesh_cases.MESHES["degenerate"]
    v2, f2 = mesh_cases.MESHES["faces65"]
    v3, f3 = _sphere(24, 16)
    instances = [(v, f, None, False, True), (v2, f2, "white", True, False), (v3, f3, "glass", False, True)]
    pose_a = [SMALL_IN_BOX, _shift(SMALL_IN_BOX, -0.3, 0.2, -0.4), _shift(IN_BOX, 0.3, -0.3, 0.3, 0.5)]
    moved = PROJECTIVE @ SMALL_IN_BOX
    pose_b = [moved, pose_a[1], pose_a[2]]
    n_a = mesh_cases.load_mesh(host, "pth_", v, f, SMALL_IN_BOX, 1)[0]
    n_b = mesh_cases.load_mesh(host, "pth_", v, f, moved, 1)[0]
    assert n_a != n_b and n_a > 0 and n_b > 0  # the count does change, by the loader's numbers
    with env(PT_BUILD=mode):
        g = binding.Scene(_mesh_scene(instances, pose_a))
        try:
            first_a, count_a = g.instance_ranges()
            g.pose([moved], instances=[0])
            first_b, count_b = g.instance_ranges()
            assert (count_a[0], count_b[0]) == (n_a, n_b) and count_a[1:].tolist() == count_b[1:].tolist()
            assert (first_b[1:].astype(np.int64) - first_a[1:].astype(np.int64)).tolist() == [n_b - n_a] * 2 and first_a[0] == first_b[0]
            _assert_posed_equals_flat(host, g, instances, pose_b, "instance 0 posed alone", spp=(4, 4))
        finally:
            g.close()


# ---- 5. no history ---------------------------------------------------------------------------------------------------------------------------

def test_a_pose_leaves_no_history(host):
    from cpupathtrace_amd import binding
    instances, pose_a, pose_b = _four_instances()
    desc_a = _mesh_scene(instances, pose_a)
    g, fresh = binding.Scene(desc_a), binding.Scene(desc_a)
    try:
        assert_bits_equal(g.pose_transforms(), np.array(pose_a, F), "pt_scene_get_pose after creation")
        first_a = _state(g)
        g.pose(pose_b)
        assert_bits_equal(g.pose_transforms(), np.array(pose_b, F), "pt_scene_get_pose after B")
        full_b = _state(g)
        g.pose(pose_a)
        assert_bits_equal(g.pose_transforms(), np.array(pose_a, F), "pt_scene_get_pose after A")
        second_a = _state(g)
        _assert_same_state(second_a, first_a, "A -> B -> A against the first A")
        _assert_same_state(second_a, _state(fresh), "A -> B -> A against a fresh scene at A")
        # a subset pose is the full pose with the other matrices unchanged; duplicates apply in order
        g.pose([pose_a[3], pose_b[3], pose_b[1]], instances=[3, 3, 1])
        g.pose([pose_b[0], pose_b[2]], instances=[0, 2])
        assert_bits_equal(g.pose_transforms(), np.array(pose_b, F), "pt_scene_get_pose after the subset poses")
        _assert_same_state(_state(g), full_b, "subset poses against the full pose")
        _assert_posed_equals_flat(host, g, instances, pose_b, "subset poses", frame=False)
    finally:
        g.close()
        fresh.close()


# ---- 6. refusals with a scene ------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_scene_as_it_was(host):
    from cpupathtrace_amd import binding
    instances, pose_a, pose_b = _four_instances()
    opt = scenes.options(64, 64, 4, 8)
    plain = binding.Scene(_flat_scene(host, instances[:1], pose_a[:1])[0])
    g = binding.Scene(_mesh_scene(instances, pose_a))
    try:
        for call in (lambda: plain.pose(pose_a[:1]), plain.pose_transforms):
            with pytest.raises(binding.PtError) as refused:
                call()
            assert refused.value.code == PT_ERR_UNSUPPORTED
        before = g.process_job(CAMERA, opt, base_seed=77)
        for matrices, index in ((pose_b[:1], [4]), (pose_b[:2], [0, 0xFFFFFFFF]), (pose_b[:3], None), (np.zeros((0, 16), F), None)):
            with pytest.raises(binding.PtError) as refused:
                g.pose(matrices, instances=index)
            assert refused.value.code == PT_ERR_INVALID
        assert_bits_equal(g.pose_transforms(), np.array(pose_a, F), "matrices after refused poses")
        assert_bits_equal(g.process_job(CAMERA, opt, base_seed=77), before, "frame after refused poses")
        # a live frame: its parked state belongs to the geometry it was created on
        frame = binding.Frame(g, CAMERA, opt, base_seed=77)
        with pytest.raises(binding.PtError) as refused:
            g.pose(pose_b)
        assert refused.value.code == PT_ERR_INVALID and "frame" in str(refused.value)
        image, _, info = frame.render()
        assert info["status"] == 0
        assert_bits_equal(image, before, "the frame of the scene that refused the pose")
        frame.close()
        g.pose(pose_b)
        # a frame created after a pose is the posed scene's
        frame = binding.Frame(g, CAMERA, opt, base_seed=77)
        try:
            image, _, info = frame.render()
            assert info["status"] == 0
            image = image.copy()
        finally:
            frame.close()
        assert_bits_equal(image, g.process_job(CAMERA, opt, base_seed=77), "a frame created after the pose")
        _assert_posed_equals_flat(host, g, instances, pose_b, "after the frame", frame=False)
    finally:
        g.close()
        plain.close()


# ---- 7. views and features after a pose --------------------------------------------------------------------------------------------------------

def test_views_and_features_after_a_pose(host):
    from cpupathtrace_amd import binding
    instances, pose_a, pose_b = _four_instances()
    g = binding.Scene(_mesh_scene(instances, pose_a))
    try:
        opt = scenes.options(64, 64, 4, 4)
        g.process_views([CAMERA, CAMERA_2], opt, base_seeds=[5, 6])
        g.render_features(CAMERA, opt, followed={})
        g.pose(pose_b)
        _assert_posed_equals_flat(host, g, instances, pose_b, "views and features", frame=False, extras=True)
    finally:
        g.close()
