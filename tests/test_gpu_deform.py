"""Deforming meshes in place (include/pt_deform.h, pt_deform.cpp, pt_deform.hip), bit for bit: the vertices the skinning kernel makes
against the NumPy restatement of the header's arithmetic (tests/deform_ref.py), and a deformed scene against a FRESH scene created from
the same description, faces, flags, materials and matrices with meshes whose vertices are what Scene.mesh_vertices() returns: info,
tree, emitters, instance ranges, triangles read back, 4096 hits, a frame and a feature frame.  No tolerance anywhere; NaN compares by
NaN-ness."""
import ctypes as C

import numpy as np
import pytest

from cpupathtrace_amd import scenes
from tests import deform_cases, deform_ref
from tests.util import assert_bits_equal, env

pytestmark = pytest.mark.gpu

F = np.float32
PT_ERR_INVALID, PT_ERR_UNSUPPORTED = 1, 4
IN_BOX = np.array(scenes.DRAGON_BOX_TRANSFORM, F)  # the bumpy sphere (radius 40 around (0, 50, 0)) into the unit box
CAMERA = scenes.camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0)
CAMERA_2 = scenes.camera((1.5, 0.5, -2.5), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0)
MATERIALS = dict(glass=dict(diffuse=(1, 1, 1, 1), ior=1.5, bsdf=scenes.BSDF_GLASS), white=dict(diffuse=(0.8, 0.7, 0.6, 1.0)),
                 lamp=dict(diffuse=(1, 1, 1, 1), emission=(1.0, 0.9, 0.8, 2.0)))
MATERIAL_ORDER = list(MATERIALS)
OPT = scenes.options(32, 32, 4, 8)


def _shift(m, dx, dy, dz, scale=1.0):
    out = np.array(m, F)
    out[:3, :3] *= F(scale)
    out[:3, 3] += np.array([dx, dy, dz], F)
    return out


def _rays(n=4096, seed=5):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([rng.uniform(-0.95, 0.95, (n, 3)), d], axis=1).astype(F)


RAYS = _rays()


def _description(meshes, instances, matrices):
    """The box of tests/test_gpu_pose.py -- walls, light quad, a sphere, a point light -- with the instances (mesh index, material name,
    cull, smooth) of `meshes` [(vertices, faces)] under `matrices`.  Mesh k of the scene is meshes[k]: the instances use them in order."""
    sb = scenes.SceneBuilder()
    sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)))
    light = sb.material((1, 1, 1, 1), 1.0, (1, 1, 1, 1))
    sb.triangles(scenes.make_plane((-0.25, F(1.0) - F(0.01), -0.25), (0.25, F(1.0) - F(0.01), 0.25)), light)
    sb.sphere((0.55, -0.7, -0.3), 0.3, sb.material((0, 0, 1, 1), bsdf=scenes.BSDF_MIRROR))
    sb.point_light((-0.6, 0.7, -0.6), (0.5, 0.5, 0.4, 1.0))
    mats = {name: sb.material(**MATERIALS[name]) for name in MATERIAL_ORDER}
    mats[None] = scenes.NO_MATERIAL
    first_use = []
    for (mesh, material, cull, smooth), m in zip(instances, matrices):
        if mesh not in first_use:
            first_use.append(mesh)
        v, f = meshes[mesh]
        sb.mesh(v, f, m, mats[material], cull=cull, smooth=smooth)
    assert first_use == sorted(first_use) == list(range(len(first_use))), "meshes are numbered by first use"
    return sb.build(), mats


def _state(g, desc, extras=False):
    """What the entry points say about a scene, as arrays: compared between scenes bit for bit."""
    out = {"info": g.info(), "n_objects": g.n_objects}
    out["bvh topology"], out["bvh boxes"] = g.bvh_dump()
    out["emitter order"], out["emitter cdf"] = g.emissive()
    out["instance first"], out["instance count"] = g.instance_ranges()
    n_desc, n_tri_desc = len(desc["obj_kind"]), len(desc["tri_pos"])
    for name, (start, length) in (("description", (0, n_tri_desc)), ("instances", (n_desc, g.n_objects - n_desc))):
        if length > 0:
            for part, a in zip(("positions", "normals", "cull", "material"), g.triangles(start, length)):
                out["get_triangles %s %s" % (name, part)] = a
    out["hit t"], out["hit object"] = g.get_intersection(RAYS)
    out["pixels"] = g.process_job(CAMERA, OPT, base_seed=77)
    out["features"] = g.render_features(CAMERA, OPT)
    if extras:
        out["views"] = g.process_views([CAMERA, CAMERA_2], OPT, base_seeds=[5, 6])
        out["followed features"] = g.render_features(CAMERA, OPT, followed={})
    return out


def _assert_same_state(a, b, what):
    assert a["info"] == b["info"] and a["n_objects"] == b["n_objects"], (what, a["info"], b["info"], a["n_objects"], b["n_objects"])
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for key in a:
        if key not in ("info", "n_objects"):
            assert_bits_equal(a[key], b[key], "%s: %s" % (what, key))


def _assert_equals_fresh(g, meshes, instances, matrices, what, extras=False, materials=None):
    """The deformed scene against a fresh one of Scene.mesh_vertices(); returns the fresh scene's state."""
    from cpupathtrace_amd import binding
    assert_bits_equal(g.pose_transforms(), np.array(matrices, F).reshape(-1, 4, 4), what + ": pt_scene_get_pose")
    current = [(g.mesh_vertices(k), f) for k, (_, f) in enumerate(meshes)]
    desc, _ = _description(current, instances, matrices)
    if materials is not None:
        desc["materials"] = materials
    fresh = binding.Scene(desc)
    try:
        for k in range(len(meshes)):
            assert_bits_equal(fresh.mesh_vertices(k), current[k][0], what + ": a fresh scene's vertices")
        want = _state(fresh, desc, extras)
        _assert_same_state(_state(g, desc, extras), want, what)
        return want
    finally:
        fresh.close()


def _sphere(nu, nv):
    v, f = scenes.bumpy_sphere_vertices(nu, nv)
    return np.array(v, F), np.array(f, np.int32)


def _three_meshes():
    """Mesh 0 (266 vertices, more than one block) under two matrices, one of its instances a lamp; mesh 1 that no deform names; mesh 2."""
    meshes = [_sphere(24, 12), _sphere(8, 4), _sphere(24, 12)]
    instances = [(0, "glass", False, True), (1, "white", True, False), (2, None, False, True), (0, "lamp", True, False)]
    pose_a = [_shift(IN_BOX, -0.4, -0.3, 0.2, 0.5), _shift(IN_BOX, 0.3, 0.1, 0.3, 0.5), _shift(IN_BOX, 0.35, -0.4, -0.3, 0.45), _shift(IN_BOX, -0.3, 0.2, -0.4, 0.4)]
    pose_b = [_shift(IN_BOX, 0.2, 0.3, -0.2, 0.4), pose_a[1], _shift(IN_BOX, -0.35, -0.2, 0.1, 0.6), _shift(IN_BOX, 0.1, -0.5, 0.3, 0.5)]
    return meshes, instances, pose_a, pose_b


def _squashed(v):
    out = np.array(v, F)
    out[:, 0] *= F(1.25)
    out[:, 1] = F(50.0) + (out[:, 1] - F(50.0)) * F(0.5)
    out[:, 2] += F(0.1) * (v[:, 1] - F(50.0))
    return out


def _bind(g, mesh, n_vertices, n_bones, k, kind="partition"):
    bone, weight = deform_cases.rig(n_vertices, n_bones, k, kind)
    g.bind_skin(mesh, bone, weight, n_bones=n_bones)
    return bone, weight


# ---- 1. the kernel's vertices ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def family_scene():
    """One small scene with a mesh per vertex-count family that fits it: 1, 255, 256 and 257 vertices (the first vertices of the
    266-vertex sphere and the faces among them), all 266, and the 26 of the small sphere.  1000 vertices are the host-compiled kernel's
    (tests/test_deform_cases_cpu.py); a last partial block and more than one block are here."""
    from cpupathtrace_amd import binding
    big, small = _sphere(24, 12), _sphere(8, 4)
    meshes = [deform_cases.truncated(big[0], big[1], n) for n in (1, 255, 256, 257)] + [big, small]
    assert [len(v) for v, _ in meshes] == [1, 255, 256, 257, 266, 26]
    instances = [(k, None, False, False) for k in range(len(meshes))]
    matrices = [_shift(IN_BOX, -0.5 + 0.2 * k, -0.2, 0.1 * k, 0.3) for k in range(len(meshes))]
    g = binding.Scene(_description(meshes, instances, matrices)[0])
    yield g, meshes
    g.close()


def _skin_all(g, meshes, n_bones, k, kind, bones):
    rigs = [_bind(g, m, len(v), n_bones, k, kind) for m, (v, _) in enumerate(meshes)]
    info = g.deform(bones={m: bones for m in range(len(meshes))})
    assert info["n_meshes_deformed"] == len(meshes) and info["n_vertices_skinned"] == sum(len(v) for v, _ in meshes)
    for m, ((v, _), (bone, weight)) in enumerate(zip(meshes, rigs)):
        assert_bits_equal(g.mesh_vertices(m), deform_ref.skin(v, bone, weight, bones),
                          "%d vertices, K=%d, %d bones, %s weights" % (len(v), k, n_bones, kind))
    return info


@pytest.mark.parametrize("k", deform_cases.INFLUENCES)
def test_skinned_vertices_equal_the_reference(family_scene, k):
    g, meshes = family_scene
    for n_bones in deform_cases.BONE_COUNTS:  # (LDS up to deform_cases.LDS_BONES, the cache beyond)
        _skin_all(g, meshes, n_bones, k, "partition", deform_cases.bone_matrices(n_bones))
    with env(PT_SKIN_LDS_BONES=0):  # the cache form at counts the LDS form takes otherwise
        for n_bones in (1, 2, deform_cases.LDS_BONES):
            _skin_all(g, meshes, n_bones, k, "partition", deform_cases.bone_matrices(n_bones, seed=7))
    for kind in ("zero", "wild", "denormal"):
        for n_bones in (2, deform_cases.LDS_BONES + 1):
            info = _skin_all(g, meshes, n_bones, k, kind, deform_cases.bone_matrices(n_bones, seed=8))
            if kind == "zero":  # every vertex at the origin: every face of every instance is rejected
                assert info["n_triangles"] == 0 and g.instance_ranges()[1].tolist() == [0] * len(meshes)


@pytest.mark.parametrize("k", deform_cases.INFLUENCES)
def test_poisoned_bones_give_nan_vertices(family_scene, k):
    g, meshes = family_scene
    for n_bones, lds in ((5, None), (5, 0), (deform_cases.LDS_BONES + 1, None)):
        bones = deform_cases.poison(deform_cases.bone_matrices(n_bones))
        rigs = [deform_cases.poisoned_rig(len(v), n_bones, k) for v, _ in meshes]
        for m, (bone, weight, _) in enumerate(rigs):
            g.bind_skin(m, bone, weight, n_bones=n_bones)
        with env(PT_SKIN_LDS_BONES=lds) if lds is not None else env():
            g.deform(bones={m: bones for m in range(len(meshes))})
        for m, ((v, _), (bone, weight, poisoned)) in enumerate(zip(meshes, rigs)):
            got = g.mesh_vertices(m)
            assert_bits_equal(got, deform_ref.skin(v, bone, weight, bones), "poisoned bones, %d vertices, K=%d, %d bones" % (len(v), k, n_bones))
            assert np.isnan(got[poisoned]).any(axis=1).all() and np.isfinite(got[~poisoned]).all()
            zero_weight = poisoned & (weight[:, k - 1] == 0)
            assert np.isnan(got[zero_weight]).any(axis=1).all()  # (no influence is skipped)


# ---- 2. a deformed scene is the fresh scene of its vertices --------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["host", "device"])
def test_deformed_scene_equals_fresh_scene(mode):
    from cpupathtrace_amd import binding
    meshes, instances, pose_a, pose_b = _three_meshes()
    with env(PT_BUILD=mode):
        desc, _ = _description(meshes, instances, pose_a)
        g = binding.Scene(desc)
        try:
            created = _state(g, desc)
            # new vertices from the caller, for mesh 0 alone
            info = g.deform(vertices={0: _squashed(meshes[0][0])})
            assert (info["n_instances"], info["n_meshes_deformed"], info["n_vertices_skinned"]) == (4, 1, 0)
            assert (info["assembly_syncs"], info["assembly_chunks"]) == (1, 1)
            assert_bits_equal(g.mesh_vertices(0), _squashed(meshes[0][0]), "the vertices handed over")
            assert_bits_equal(g.mesh_vertices(1), meshes[1][0], "a mesh no deform names")
            assert_bits_equal(g.mesh_vertices(2), meshes[2][0], "a mesh no deform names")
            vertices_state = _assert_equals_fresh(g, meshes, instances, pose_a, "vertices deform, PT_BUILD=%s" % mode)
            assert not np.array_equal(vertices_state["pixels"], created["pixels"])
            # bones for meshes 0 and 2, mesh 1 between them unnamed: its pointer stays the rest vertices
            rig_0 = _bind(g, 0, len(meshes[0][0]), 6, 4)
            rig_2 = _bind(g, 2, len(meshes[2][0]), 3, 3)
            bones_0, bones_2 = deform_cases.bone_matrices(6, seed=21), deform_cases.bone_matrices(3, seed=22)
            _assert_same_state(_state(g, desc), vertices_state, "binding changes no geometry")
            info = g.deform(bones={0: bones_0, 2: bones_2})
            assert (info["n_meshes_deformed"], info["n_vertices_skinned"]) == (2, len(meshes[0][0]) + len(meshes[2][0]))
            assert_bits_equal(g.mesh_vertices(0), deform_ref.skin(meshes[0][0], *rig_0, bones_0), "mesh 0 skinned from the REST vertices")
            assert_bits_equal(g.mesh_vertices(2), deform_ref.skin(meshes[2][0], *rig_2, bones_2), "mesh 2 skinned")
            assert_bits_equal(g.mesh_vertices(1), meshes[1][0], "the unnamed mesh between two named ones")
            _assert_equals_fresh(g, meshes, instances, pose_a, "bones deform, PT_BUILD=%s" % mode)
            # a deform with new matrices in the same call, one mesh by vertices and one by bones
            bones_0b = deform_cases.bone_matrices(6, seed=23)
            info = g.deform(vertices={2: _squashed(meshes[2][0])}, bones={0: bones_0b}, transforms=pose_b)
            assert info["n_meshes_deformed"] == 2 and info["n_vertices_skinned"] == len(meshes[0][0])
            assert_bits_equal(g.mesh_vertices(0), deform_ref.skin(meshes[0][0], *rig_0, bones_0b), "mesh 0 skinned again")
            _assert_equals_fresh(g, meshes, instances, pose_b, "deform with new matrices, PT_BUILD=%s" % mode)
            # matrices for two instances only, no mesh named
            g.deform(transforms=[pose_a[3], pose_a[0]], instances=[3, 0])
            mixed = [pose_a[0], pose_b[1], pose_b[2], pose_a[3]]
            _assert_equals_fresh(g, meshes, instances, mixed, "deform of matrices alone, PT_BUILD=%s" % mode)
            # REST after the deforms: the scene as created
            info = g.deform(rest=[0, 2], transforms=pose_a)
            assert (info["n_meshes_deformed"], info["n_vertices_skinned"]) == (2, 0)
            for k in range(3):
                assert_bits_equal(g.mesh_vertices(k), meshes[k][0], "the rest vertices")
            _assert_same_state(_state(g, desc), created, "REST equals the scene as created, PT_BUILD=%s" % mode)
        finally:
            g.close()


def test_a_mesh_named_twice_takes_its_last_entry():
    from cpupathtrace_amd import binding
    meshes, instances, pose_a, _ = _three_meshes()
    g = binding.Scene(_description(meshes, instances, pose_a)[0])
    try:
        v1, v2 = _squashed(meshes[0][0]), _squashed(_squashed(meshes[0][0]))
        table = (binding.MeshDeform * 3)(binding.MeshDeform(0, binding.DEFORM_VERTICES, v1.ctypes.data, len(v1)), binding.MeshDeform(0, binding.DEFORM_REST, None, 0),
                                         binding.MeshDeform(0, binding.DEFORM_VERTICES, v2.ctypes.data, len(v2)))
        info = binding.DeformInfo()
        assert binding.load().pt_scene_deform(g._h, table, C.c_uint32(3), None, C.c_uint32(0), None, C.byref(info)) == 0
        assert info.n_meshes_deformed == 1
        assert_bits_equal(g.mesh_vertices(0), v2, "the last entry")
    finally:
        g.close()


# ---- 3. emitters follow the rejected faces -----------------------------------------------------------------------------------------------------

def test_emitters_and_ranges_follow_rejected_faces():
    """Mesh 0 has a lamp instance.  Bones with a NaN and an infinite entry make NaN vertices, the assembler's face test rejects their
    faces: survivor counts drop, the ranges behind move, and the emitter registry holds the lamp's survivors only."""
    from cpupathtrace_amd import binding
    meshes, instances, pose_a, _ = _three_meshes()
    n_vertices = len(meshes[0][0])
    g = binding.Scene(_description(meshes, instances, pose_a)[0])
    try:
        first_a, count_a = g.instance_ranges()
        count_a = [int(c) for c in count_a]
        assert g.info()["n_emissive"] == 2 + count_a[3]
        bone, weight, poisoned = deform_cases.poisoned_rig(n_vertices, 8, 4)
        g.bind_skin(0, bone, weight, n_bones=8)
        healthy = deform_cases.bone_matrices(8, seed=31, scale=0.05, shift=1.0)
        g.deform(bones={0: healthy})
        first_h, count_h = g.instance_ranges()
        assert count_h.tolist() == count_a  # (a gentle rig rejects nothing)
        g.deform(bones={0: deform_cases.poison(healthy)})
        got = g.mesh_vertices(0)
        assert np.isnan(got[poisoned]).any(axis=1).all() and np.isfinite(got[~poisoned]).all()
        # the faces that survive are those without a poisoned corner, by the mesh's own indices
        survivors = int((~poisoned[meshes[0][1]].any(axis=1)).sum())
        first_b, count_b = g.instance_ranges()
        assert 0 < survivors < len(meshes[0][1]) and count_b.tolist() == [survivors, count_a[1], count_a[2], survivors]
        assert (first_b.astype(np.int64) - first_a.astype(np.int64)).tolist() == [0, survivors - count_a[0], survivors - count_a[0], survivors - count_a[0]]
        assert g.info()["n_emissive"] == 2 + survivors
        state = _assert_equals_fresh(g, meshes, instances, pose_a, "poisoned bones")
        assert len(state["emitter order"]) == 2 + survivors
        # all weights zero: the instances of mesh 0 vanish, the others stay
        g.bind_skin(0, bone, np.zeros_like(weight), n_bones=8)
        info = g.deform(bones={0: healthy})
        assert g.instance_ranges()[1].tolist() == [0, count_a[1], count_a[2], 0] and info["n_triangles"] == count_a[1] + count_a[2]
        assert g.info()["n_emissive"] == 2
        _assert_equals_fresh(g, meshes, instances, pose_a, "all weights zero")
    finally:
        g.close()


# ---- 4. pose and relight after a deform -------------------------------------------------------------------------------------------------------

def test_pose_and_relight_keep_the_deformed_shape():
    from cpupathtrace_amd import binding
    meshes, instances, pose_a, pose_b = _three_meshes()
    desc, mats = _description(meshes, instances, pose_a)
    g = binding.Scene(desc)
    try:
        rig = _bind(g, 0, len(meshes[0][0]), 4, 3)
        bones = deform_cases.bone_matrices(4, seed=41)
        g.deform(bones={0: bones}, vertices={2: _squashed(meshes[2][0])})
        skinned = deform_ref.skin(meshes[0][0], *rig, bones)
        g.pose(pose_b)
        assert_bits_equal(g.mesh_vertices(0), skinned, "vertices after a pose")
        _assert_equals_fresh(g, meshes, instances, pose_b, "pose after deform")
        g.pose([pose_a[3]], instances=[3])
        _assert_equals_fresh(g, meshes, instances, pose_b[:3] + [pose_a[3]], "subset pose after deform")
        # relight: instance 0 becomes a lamp, the white material turns red
        table = g.materials()
        table[mats["white"]]["diffuse"] = (0.9, 0.1, 0.1, 1.0)
        g.relight(materials=table, instance_materials={0: mats["lamp"]})
        relit = [(0, "lamp", False, True)] + instances[1:]
        assert_bits_equal(g.mesh_vertices(0), skinned, "vertices after a relight")
        _assert_equals_fresh(g, meshes, relit, pose_b[:3] + [pose_a[3]], "relight after deform", materials=table)
    finally:
        g.close()


# ---- 5. no compounding, no allocation -----------------------------------------------------------------------------------------------------

def test_two_bones_deforms_equal_the_second_alone():
    from cpupathtrace_amd import binding
    meshes, instances, pose_a, _ = _three_meshes()
    desc, _ = _description(meshes, instances, pose_a)
    g, alone = binding.Scene(desc), binding.Scene(desc)
    try:
        first, second = deform_cases.bone_matrices(5, seed=51), deform_cases.bone_matrices(5, seed=52)
        for scene in (g, alone):
            _bind(scene, 0, len(meshes[0][0]), 5, 4)
        info_1 = g.deform(bones={0: first})
        info_2 = g.deform(bones={0: second})
        info_3 = g.deform(bones={0: first})
        info_4 = g.deform(bones={0: second})
        alone.deform(bones={0: second})
        assert_bits_equal(g.mesh_vertices(0), alone.mesh_vertices(0), "skinning never compounds")
        _assert_same_state(_state(g, desc), _state(alone, desc), "two deforms against the second alone")
        # buffers and scratch come with the first deformation: the later ones allocate nothing
        assert info_1["allocations"] > 0
        assert info_2["allocations"] == info_3["allocations"] == info_4["allocations"] == info_1["allocations"], (info_1, info_2, info_3, info_4)
    finally:
        g.close()
        alone.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_scene_and_the_vertices_as_they_were():
    from cpupathtrace_amd import binding
    meshes, instances, pose_a, pose_b = _three_meshes()
    desc, _ = _description(meshes, instances, pose_a)
    g = binding.Scene(desc)
    plain = binding.Scene(scenes.box_scene()[0])
    try:
        for call in (lambda: plain.deform(rest=[0]), lambda: plain.mesh_vertices(0), lambda: plain.bind_skin(0, np.zeros((1, 1), np.uint32), np.ones((1, 1), F))):
            with pytest.raises(binding.PtError) as refused:
                call()
            assert refused.value.code == PT_ERR_UNSUPPORTED
        n0 = len(meshes[0][0])
        rig = _bind(g, 0, n0, 4, 2)
        bones = deform_cases.bone_matrices(4, seed=61)
        g.deform(bones={0: bones}, vertices={2: _squashed(meshes[2][0])})
        before = _state(g, desc)
        vertices = [g.mesh_vertices(k) for k in range(3)]

        def unchanged(what):
            for k in range(3):
                assert_bits_equal(g.mesh_vertices(k), vertices[k], what + ": vertices of mesh %d" % k)
            assert_bits_equal(g.pose_transforms(), np.array(pose_a, F), what + ": matrices")
            _assert_same_state(_state(g, desc), before, what)

        other = deform_cases.bone_matrices(4, seed=62)
        bad_bone = np.array(rig[0])
        bad_bone[n0 // 2, 1] = 4  # a bone index equal to n_bones
        refusals = {
            "bones without a skin": lambda: g.deform(bones={2: other}),
            "a wrong bone count": lambda: g.deform(bones={0: deform_cases.bone_matrices(5)}),
            "a wrong vertex count": lambda: g.deform(vertices={0: meshes[0][0][:-1]}),
            "a wrong vertex count behind a good entry": lambda: g.deform(bones={0: other}, vertices={2: meshes[1][0]}),
            "a mesh out of range": lambda: g.deform(rest=[3]),
            "new matrices that name a bad instance": lambda: g.deform(bones={0: other}, transforms=[pose_b[0]], instances=[4]),
            "matrices for some instances without their indices": lambda: g.deform(bones={0: other}, transforms=pose_b[:3]),
            "a bone index equal to n_bones": lambda: g.bind_skin(0, bad_bone, rig[1], n_bones=4),
            "nine influences": lambda: g.bind_skin(0, np.zeros((n0, 9), np.uint32), np.zeros((n0, 9), F), n_bones=4),
            "a skin for a mesh out of range": lambda: g.bind_skin(3, rig[0], rig[1], n_bones=4),
        }
        for what, call in refusals.items():
            with pytest.raises(binding.PtError) as refused:
                call()
            assert refused.value.code == PT_ERR_INVALID, what
        unchanged("after the refusals")
        # (the refused bind left the skin of mesh 0 bound: the same bones give the same vertices)
        g.deform(bones={0: bones})
        unchanged("the skin survived the refused binds")
        # a live frame: its parked state belongs to the geometry it was created on
        frame = binding.Frame(g, CAMERA, OPT, base_seed=77)
        for call in (lambda: g.deform(bones={0: other}), lambda: g.deform(rest=[0]), lambda: g.bind_skin(0, rig[0], rig[1], n_bones=4)):
            with pytest.raises(binding.PtError) as refused:
                call()
            assert refused.value.code == PT_ERR_INVALID and "frame" in str(refused.value)
        image, _, info = frame.render()
        assert info["status"] == 0
        assert_bits_equal(image, before["pixels"], "the frame of the scene that refused the deform")
        frame.close()
        unchanged("after the live frame")
        g.deform(bones={0: other})
        assert_bits_equal(g.mesh_vertices(0), deform_ref.skin(meshes[0][0], *rig, other), "a deform once the frame is gone")
    finally:
        g.close()
        plain.close()


# ---- 7. views and features after a deform ------------------------------------------------------------------------------------------------------

def test_views_and_features_after_a_deform():
    from cpupathtrace_amd import binding
    meshes, instances, pose_a, pose_b = _three_meshes()
    g = binding.Scene(_description(meshes, instances, pose_a)[0])
    try:
        g.process_views([CAMERA, CAMERA_2], OPT, base_seeds=[5, 6])
        g.render_features(CAMERA, OPT, followed={})
        _bind(g, 0, len(meshes[0][0]), 7, 8)
        g.deform(bones={0: deform_cases.bone_matrices(7, seed=71)}, transforms=pose_b)
        _assert_equals_fresh(g, meshes, instances, pose_b, "views and features", extras=True)
    finally:
        g.close()
