"""Blend shapes in place (include/pt_morph.h, pt_morph.cpp, pt_deform.hip), bit for bit: the vertices the morph kernel makes -- alone and
in front of the bound rig -- against the NumPy restatement of the header's arithmetic (tests/morph_ref.py, tests/deform_ref.py), and a
morphed scene against a FRESH scene created from the same description, faces, flags, materials and matrices with meshes whose vertices
are what Scene.mesh_vertices() returns: info, tree, emitters, instance ranges, triangles read back, 4096 hits, a frame and a feature
frame (the comparison of tests/test_gpu_deform.py).  No tolerance anywhere; NaN compares by NaN-ness."""
import ctypes as C

import numpy as np
import pytest

from tests import deform_cases, deform_ref, morph_cases, morph_ref
from tests.test_gpu_deform import CAMERA, IN_BOX, OPT, _assert_equals_fresh, _assert_same_state, _bind, _description, _shift, _sphere, _squashed, _state, _three_meshes
from tests.util import assert_bits_equal, env

pytestmark = pytest.mark.gpu

F = np.float32
PT_ERR_INVALID, PT_ERR_UNSUPPORTED = 1, 4


# ---- 1. the kernel's vertices ------------------------------------------------------------------------------------------------------------------

def _family_scene():
    """One small scene with a mesh per vertex-count family that fits it: 1, 255, 256 and 257 vertices (the first vertices of the
    266-vertex sphere and the faces among them), all 266, and the 26 of the small sphere.  1000 vertices are the host-compiled kernel's
    (tests/test_morph_cases_cpu.py); a last partial block and more than one block are here."""
    from cpupathtrace_amd import binding
    big, small = _sphere(24, 12), _sphere(8, 4)
    meshes = [deform_cases.truncated(big[0], big[1], n) for n in (1, 255, 256, 257)] + [big, small]
    assert [len(v) for v, _ in meshes] == [1, 255, 256, 257, 266, 26]
    instances = [(k, None, False, False) for k in range(len(meshes))]
    matrices = [_shift(IN_BOX, -0.5 + 0.2 * k, -0.2, 0.1 * k, 0.3) for k in range(len(meshes))]
    return binding.Scene(_description(meshes, instances, matrices)[0]), meshes


@pytest.fixture(scope="module")
def family_scene():
    g, meshes = _family_scene()
    yield g, meshes
    g.close()


_SETS, _MORPHED = {}, {}  # the families' sets and their morphed vertices, made once and shared by the cases below; never written again


def _set_of(n_vertices, n_targets, form):
    key = (n_vertices, n_targets, form)
    if key not in _SETS:
        _SETS[key] = morph_cases.target_set(n_vertices, n_targets, form)
    return _SETS[key]


def _morphed(v, n_targets, form, kind):
    """morph_ref.morph of the family's set over the first len(v) vertices of the sphere under the family's weights."""
    key = (len(v), n_targets, form, kind)
    if key not in _MORPHED:
        _MORPHED[key] = morph_ref.morph(v, _set_of(len(v), n_targets, form), morph_cases.weights(n_targets, kind))
    return _MORPHED[key]


def _bind_sets(g, meshes, n_targets, form):
    sets = [_set_of(len(v), n_targets, form) for v, _ in meshes]
    for m, targets in enumerate(sets):
        g.bind_morphs(m, targets)
        assert g.morphs(m) == (n_targets, sum(len(d) for _, d in targets))
    return sets


def _bind_skins(g, meshes, k, n_bones):
    if k == 0:
        return None, None
    rigs = [_bind(g, m, len(v), n_bones, k) for m, (v, _) in enumerate(meshes)]
    return rigs, deform_cases.bone_matrices(n_bones)


def _morph_all(g, meshes, sets, weights, rigs, bones, what, morphed=None):
    every = range(len(meshes))
    info = g.morph(weights={m: weights for m in every}, bones=None if rigs is None else {m: bones for m in every})
    n_all = sum(len(v) for v, _ in meshes)
    assert (info["n_meshes_deformed"], info["n_vertices_morphed"], info["n_vertices_skinned"]) == (len(meshes), n_all, 0 if rigs is None else n_all)
    assert info["n_entries_read"] == sum(len(d) for targets in sets for _, d in targets)
    for m, (v, _) in enumerate(meshes):
        want = morph_ref.morph(v, sets[m], weights) if morphed is None else morphed[m]
        if rigs is not None:
            want = deform_ref.skin(want, *rigs[m], bones)
        assert_bits_equal(g.mesh_vertices(m), want, "%d vertices, %s" % (len(v), what))
    return info


@pytest.mark.parametrize("k,n_bones", morph_cases.SKINS)
def test_morphed_vertices_equal_the_reference(family_scene, k, n_bones):
    g, meshes = family_scene
    rigs, bones = _bind_skins(g, meshes, k, n_bones)
    for n_targets in morph_cases.TARGET_COUNTS:  # (weights in LDS up to morph_cases.LDS_TARGETS and 256 bones, the cache beyond either)
        for form in morph_cases.FORMS:
            sets = _bind_sets(g, meshes, n_targets, form)
            kinds = morph_cases.WEIGHT_KINDS if form == "sparse" and n_targets in (3, morph_cases.LDS_TARGETS + 1) else ("partition",)
            for kind in kinds:
                what = "%d %s targets, %s weights, K=%d, %d bones" % (n_targets, form, kind, k, n_bones)
                _morph_all(g, meshes, sets, morph_cases.weights(n_targets, kind), rigs, bones, what, [_morphed(v, n_targets, form, kind) for v, _ in meshes])


@pytest.mark.parametrize("k,n_bones", [(0, 0), (4, 2)])
def test_the_cache_form_at_counts_the_lds_form_takes(k, n_bones):
    with env(PT_MORPH_LDS_TARGETS=0):
        g, meshes = _family_scene()  # a fresh scene under the variable
        try:
            rigs, bones = _bind_skins(g, meshes, k, n_bones)
            for n_targets, form in ((1, "dense"), (3, "sparse"), (3, "mixed"), (morph_cases.LDS_TARGETS, "sparse")):
                sets = _bind_sets(g, meshes, n_targets, form)
                _morph_all(g, meshes, sets, morph_cases.weights(n_targets, "wild"), rigs, bones, "cache form, %d %s targets, K=%d" % (n_targets, form, k),
                           [_morphed(v, n_targets, form, "wild") for v, _ in meshes])
        finally:
            g.close()


@pytest.mark.parametrize("k,n_bones", [(0, 0), (4, 2), (8, 257)])
def test_poisoned_deltas_give_nan_vertices(family_scene, k, n_bones):
    g, meshes = family_scene
    rigs, bones = _bind_skins(g, meshes, k, n_bones)
    cases = [morph_cases.poisoned_set(len(v)) for v, _ in meshes]
    for m, (targets, _) in enumerate(cases):
        g.bind_morphs(m, targets)
    for kind, lds in (("partition", None), ("zero", None), ("zero", 0)):
        w = morph_cases.weights(len(cases[0][0]), kind)
        with env(PT_MORPH_LDS_TARGETS=lds) if lds is not None else env():
            g.morph(weights={m: w for m in range(len(meshes))}, bones=None if rigs is None else {m: bones for m in range(len(meshes))})
        for m, ((v, _), (targets, poisoned)) in enumerate(zip(meshes, cases)):
            morphed = morph_ref.morph(v, targets, w)
            want = morphed if rigs is None else deform_ref.skin(morphed, *rigs[m], bones)
            got = g.mesh_vertices(m)
            assert_bits_equal(got, want, "poisoned deltas, %d vertices, %s weights, K=%d" % (len(v), kind, k))
            assert np.isfinite(got[~poisoned]).all() and not np.isfinite(got[poisoned]).all(axis=1).any()
            if kind == "zero":
                assert np.isnan(got[poisoned]).any(axis=1).all()  # (no listed target is skipped: 0 * inf, 0 * NaN)


def test_signed_zero():
    """A mesh whose rest vertices are all -0.0: +0.0 where a zero-weight target lists the vertex, -0.0 where none does."""
    from cpupathtrace_amd import binding
    rest, targets, w, listed = morph_cases.signed_zero_case(257)
    big = _sphere(24, 12)
    _, faces = deform_cases.truncated(big[0], big[1], 257)
    meshes = [big, (rest, faces)]
    instances = [(0, None, False, False), (1, None, False, False)]
    matrices = [_shift(IN_BOX, -0.3, 0.0, 0.0, 0.4), _shift(IN_BOX, 0.3, 0.0, 0.0, 0.4)]
    for lds in (None, 0):
        with env(PT_MORPH_LDS_TARGETS=lds) if lds is not None else env():
            g = binding.Scene(_description(meshes, instances, matrices)[0])
            try:
                assert g.instance_ranges()[1].tolist()[1] == 0  # (every face of the zero mesh is degenerate)
                g.bind_morphs(1, targets)
                g.morph(weights={1: w})
                got = g.mesh_vertices(1)
                assert_bits_equal(got, morph_ref.morph(rest, targets, w), "signed zero, budget %s" % lds)
                assert (got == 0).all() and np.signbit(got[~listed]).all() and not np.signbit(got[listed]).any()
            finally:
                g.close()


# ---- 2. a morphed scene is the fresh scene of its vertices ----------------------------------------------------------------------------------

def _face_targets(v):
    """Three targets for a sphere mesh: a dense stretch, an empty one, and a sparse one that COLLAPSES the upper half: its delta is minus
    the rest vertex, so weight 1 sends every listed vertex to the origin (x + 1 * (-x) = 0 exactly) and the faces among them degenerate."""
    stretch = np.stack([F(0.25) * v[:, 0] * (v[:, 1] - F(10.0)) / F(80.0), np.zeros(len(v), F), F(0.05) * v[:, 2]], axis=1).astype(F)
    upper = np.flatnonzero(v[:, 1] > 50.0).astype(np.uint32)
    return [(None, stretch), (np.zeros(0, np.uint32), np.zeros((0, 3), F)), (upper, -v[upper])]


@pytest.mark.parametrize("mode", ["host", "device"])
def test_morphed_scene_equals_fresh_scene(mode):
    from cpupathtrace_amd import binding
    meshes, instances, pose_a, pose_b = _three_meshes()  # (mesh 0 has a glass and a lamp instance)
    with env(PT_BUILD=mode):
        desc, mats = _description(meshes, instances, pose_a)
        g = binding.Scene(desc)
        try:
            created = _state(g, desc)
            sets = {m: _face_targets(meshes[m][0]) for m in (0, 2)}
            for m, targets in sets.items():
                g.bind_morphs(m, targets)
            _assert_same_state(_state(g, desc), created, "binding changes no geometry")
            # the morph alone, mesh 0 only
            w0 = np.array([0.8, 5.0, 0.0], F)
            info = g.morph(weights={0: w0})
            assert (info["n_instances"], info["n_meshes_deformed"], info["n_vertices_morphed"], info["n_vertices_skinned"]) == (4, 1, len(meshes[0][0]), 0)
            assert (info["assembly_syncs"], info["assembly_chunks"]) == (1, 1)
            assert_bits_equal(g.mesh_vertices(0), morph_ref.morph(meshes[0][0], sets[0], w0), "mesh 0 morphed")
            assert_bits_equal(g.mesh_vertices(1), meshes[1][0], "a mesh no morph names")
            assert_bits_equal(g.mesh_vertices(2), meshes[2][0], "a mesh no morph names")
            alone = _assert_equals_fresh(g, meshes, instances, pose_a, "morph alone, PT_BUILD=%s" % mode)
            assert not np.array_equal(alone["pixels"], created["pixels"])
            # morph + bones for mesh 0, the morph alone for mesh 2, mesh 1 between them unnamed
            rig = _bind(g, 0, len(meshes[0][0]), 6, 4)
            bones = deform_cases.bone_matrices(6, seed=21)
            w0b, w2 = np.array([-0.5, 0.0, 0.25], F), np.array([1.5, 1.0, 0.0], F)
            info = g.morph(weights={0: w0b, 2: w2}, bones={0: bones})
            assert (info["n_meshes_deformed"], info["n_vertices_morphed"], info["n_vertices_skinned"]) == (2, len(meshes[0][0]) + len(meshes[2][0]), len(meshes[0][0]))
            assert_bits_equal(g.mesh_vertices(0), morph_ref.morph_skin(meshes[0][0], sets[0], w0b, *rig, bones), "mesh 0 morphed from REST, then skinned")
            assert_bits_equal(g.mesh_vertices(2), morph_ref.morph(meshes[2][0], sets[2], w2), "mesh 2 morphed")
            assert_bits_equal(g.mesh_vertices(1), meshes[1][0], "the unnamed mesh between two named ones")
            _assert_equals_fresh(g, meshes, instances, pose_a, "morph + bones, PT_BUILD=%s" % mode)
            # new matrices in the same call
            bones_b = deform_cases.bone_matrices(6, seed=23)
            g.morph(weights={0: w0}, bones={0: bones_b}, transforms=pose_b)
            assert_bits_equal(g.mesh_vertices(0), morph_ref.morph_skin(meshes[0][0], sets[0], w0, *rig, bones_b), "mesh 0 again")
            _assert_equals_fresh(g, meshes, instances, pose_b, "morph with new matrices, PT_BUILD=%s" % mode)
            # the collapsing target at weight 1: the upper half of mesh 0 -- one of its instances a lamp -- goes to the origin, the faces
            # among those vertices are rejected, ranges and emitters follow
            first_a, count_a = created["instance first"], created["instance count"]
            info = g.morph(weights={0: np.array([0.0, 0.0, 1.0], F)}, transforms=pose_a)
            got = g.mesh_vertices(0)
            upper = sets[0][2][0]
            assert (got[upper] == 0).all() and not np.signbit(got[upper]).any()
            # (at least the faces with all three corners there; which others the face test rejects is the fresh scene's to say)
            collapsed = int(np.isin(meshes[0][1], upper).all(axis=1).sum())
            survivors = int(g.instance_ranges()[1][0])
            assert collapsed > 0 and 0 < survivors <= int(count_a[0]) - collapsed
            assert g.instance_ranges()[1].tolist() == [survivors, int(count_a[1]), int(count_a[2]), survivors]
            assert g.info()["n_emissive"] == 2 + survivors and int(count_a[3]) > survivors and info["n_triangles"] == 2 * survivors + int(count_a[1]) + int(count_a[2])
            _assert_equals_fresh(g, meshes, instances, pose_a, "collapsed lamp faces, PT_BUILD=%s" % mode)
            # a later pose and relight work on the morphed shape
            g.morph(weights={0: w0b, 2: w2}, bones={0: bones})
            shape_0 = g.mesh_vertices(0)
            g.pose(pose_b)
            assert_bits_equal(g.mesh_vertices(0), shape_0, "vertices after a pose")
            _assert_equals_fresh(g, meshes, instances, pose_b, "pose after morph, PT_BUILD=%s" % mode)
            table = g.materials()
            table[mats["white"]]["diffuse"] = (0.9, 0.1, 0.1, 1.0)
            g.relight(materials=table, instance_materials={0: mats["lamp"]})
            relit = [(0, "lamp", False, True)] + instances[1:]
            assert_bits_equal(g.mesh_vertices(0), shape_0, "vertices after a relight")
            _assert_equals_fresh(g, meshes, relit, pose_b, "relight after morph, PT_BUILD=%s" % mode, materials=table)
            # back to the created shape through the deform entry: the scene a fresh one of the rest vertices is, under the new look
            info = g.deform(rest=[0, 2], transforms=pose_a)
            assert (info["n_meshes_deformed"], info["n_vertices_skinned"]) == (2, 0)
            for m in range(3):
                assert_bits_equal(g.mesh_vertices(m), meshes[m][0], "the rest vertices")
            rest_state = _assert_equals_fresh(g, meshes, relit, pose_a, "REST after the morphs, PT_BUILD=%s" % mode, materials=table)
            for key in ("bvh topology", "bvh boxes", "instance first", "instance count", "hit t", "hit object"):
                assert_bits_equal(rest_state[key], created[key], "REST equals the geometry as created: " + key)
        finally:
            g.close()


# ---- 3. the neighbours: bones alone, a mesh named twice, repeated calls -----------------------------------------------------------------------

def test_bones_alone_after_a_morph_still_skin_rest_and_nothing_compounds():
    from cpupathtrace_amd import binding
    meshes, instances, pose_a, _ = _three_meshes()
    desc, _ = _description(meshes, instances, pose_a)
    g, alone = binding.Scene(desc), binding.Scene(desc)
    try:
        targets = _face_targets(meshes[0][0])
        rigs = [_bind(scene, 0, len(meshes[0][0]), 5, 4) for scene in (g, alone)]
        bones = deform_cases.bone_matrices(5, seed=51)
        for scene in (g, alone):
            scene.bind_morphs(0, targets)
        w1, w2 = np.array([1.0, 2.0, 0.5], F), np.array([-0.3, 0.0, 0.1], F)
        info_1 = g.morph(weights={0: w1}, bones={0: bones})
        g.deform(bones={0: bones})
        assert_bits_equal(g.mesh_vertices(0), deform_ref.skin(meshes[0][0], *rigs[0], bones), "PT_DEFORM_BONES after a morph skins REST")
        info_2 = g.morph(weights={0: w2}, bones={0: bones})
        info_3 = g.morph(weights={0: w1})
        info_4 = g.morph(weights={0: w2}, bones={0: bones})
        alone.morph(weights={0: w2}, bones={0: bones})
        assert_bits_equal(g.mesh_vertices(0), alone.mesh_vertices(0), "a morph never compounds")
        assert_bits_equal(g.mesh_vertices(0), morph_ref.morph_skin(meshes[0][0], targets, w2, *rigs[0], bones), "the last call from REST")
        _assert_same_state(_state(g, desc), _state(alone, desc), "four calls against the last alone")
        # buffers and scratch come with the first call: the later ones allocate nothing
        assert info_1["allocations"] > 0
        assert info_2["allocations"] == info_3["allocations"] == info_4["allocations"] == info_1["allocations"], (info_1, info_2, info_3, info_4)
    finally:
        g.close()
        alone.close()


def test_a_mesh_named_twice_takes_its_last_entry():
    from cpupathtrace_amd import binding
    meshes, instances, pose_a, _ = _three_meshes()
    g = binding.Scene(_description(meshes, instances, pose_a)[0])
    try:
        targets = _face_targets(meshes[0][0])
        g.bind_morphs(0, targets)
        rig = _bind(g, 0, len(meshes[0][0]), 3, 2)
        bones = np.ascontiguousarray(deform_cases.bone_matrices(3, seed=5)).reshape(-1, 12)
        w1, w2 = np.array([1.0, 0.0, 0.0], F), np.array([0.2, 0.0, 0.4], F)
        table = (binding.MeshMorph * 3)(binding.MeshMorph(0, w1.ctypes.data, 3, None, 0), binding.MeshMorph(0, w1.ctypes.data, 3, bones.ctypes.data, 3),
                                        binding.MeshMorph(0, w2.ctypes.data, 3, None, 0))
        info = binding.MorphInfo()
        assert binding.load().pt_scene_morph(g._h, table, C.c_uint32(3), None, C.c_uint32(0), None, C.byref(info)) == 0
        assert (info.n_meshes_deformed, info.n_vertices_morphed, info.n_vertices_skinned) == (1, len(meshes[0][0]), 0)
        assert_bits_equal(g.mesh_vertices(0), morph_ref.morph(meshes[0][0], targets, w2), "the last entry")
        del rig
    finally:
        g.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_scene_and_the_vertices_as_they_were():
    from cpupathtrace_amd import binding, scenes
    meshes, instances, pose_a, pose_b = _three_meshes()
    desc, _ = _description(meshes, instances, pose_a)
    g = binding.Scene(desc)
    plain = binding.Scene(scenes.box_scene()[0])
    try:
        empty = (np.zeros(0, np.uint32), np.zeros((0, 3), F))
        for call in (lambda: plain.morph(weights={0: np.zeros(1, F)}), lambda: plain.morphs(0), lambda: plain.bind_morphs(0, [empty])):
            with pytest.raises(binding.PtError) as refused:
                call()
            assert refused.value.code == PT_ERR_UNSUPPORTED
        n0 = len(meshes[0][0])
        targets = _face_targets(meshes[0][0])
        g.bind_morphs(0, targets)
        rig = _bind(g, 0, n0, 4, 2)
        bones = deform_cases.bone_matrices(4, seed=61)
        w = np.array([0.7, 1.0, 0.1], F)
        g.morph(weights={0: w}, bones={0: bones})
        g.deform(vertices={2: _squashed(meshes[2][0])})
        before = _state(g, desc)
        vertices = [g.mesh_vertices(k) for k in range(3)]
        assert g.morphs(0) == (3, sum(len(d) for _, d in targets)) and g.morphs(1) == (0, 0)

        def unchanged(what):
            for k in range(3):
                assert_bits_equal(g.mesh_vertices(k), vertices[k], what + ": vertices of mesh %d" % k)
            assert_bits_equal(g.pose_transforms(), np.array(pose_a, F), what + ": matrices")
            _assert_same_state(_state(g, desc), before, what)

        other = np.array([0.1, 0.2, 0.3], F)
        delta = np.ones((2, 3), F)
        refusals = {
            "a mesh without a set": lambda: g.morph(weights={2: other}),
            "a wrong weight count": lambda: g.morph(weights={0: other[:2]}),
            "a mesh without a set behind a good entry": lambda: g.morph(weights={0: other, 2: other}),
            "a wrong bone count": lambda: g.morph(weights={0: other}, bones={0: deform_cases.bone_matrices(5)}),
            "a mesh out of range": lambda: g.morph(weights={3: other}),
            "new matrices that name a bad instance": lambda: g.morph(weights={0: other}, transforms=[pose_b[0]], instances=[4]),
            "matrices for some instances without their indices": lambda: g.morph(weights={0: other}, transforms=pose_b[:3]),
            "a vertex index equal to n_vertices": lambda: g.bind_morphs(0, [(np.array([0, n0], np.uint32), delta)]),
            "indices that do not ascend": lambda: g.bind_morphs(0, [(np.array([5, 5], np.uint32), delta)]),
            "a dense target of another length": lambda: g.bind_morphs(0, [(None, np.ones((n0 - 1, 3), F))]),
            "a set for a mesh out of range": lambda: g.bind_morphs(3, targets),
        }
        for what, call in refusals.items():
            with pytest.raises(binding.PtError) as refused:
                call()
            assert refused.value.code == PT_ERR_INVALID, what
        unchanged("after the refusals")
        g.bind_morphs(2, [empty])
        with pytest.raises(binding.PtError) as refused:
            g.morph(weights={2: np.zeros(1, F)}, bones={2: bones})  # bones without a skin
        assert refused.value.code == PT_ERR_INVALID and "skin" in str(refused.value)
        g.bind_morphs(2, None)
        unchanged("after bones without a skin")
        # (the refused binds left the set of mesh 0 bound: the same weights give the same vertices)
        assert g.morphs(0) == (3, sum(len(d) for _, d in targets))
        g.morph(weights={0: w}, bones={0: bones})
        unchanged("the set survived the refused binds")
        # a live frame: its parked state belongs to the geometry it was created on
        frame = binding.Frame(g, CAMERA, OPT, base_seed=77)
        for call in (lambda: g.morph(weights={0: other}), lambda: g.morph(weights={0: other}, bones={0: bones}), lambda: g.bind_morphs(0, targets), lambda: g.bind_morphs(0, None)):
            with pytest.raises(binding.PtError) as refused:
                call()
            assert refused.value.code == PT_ERR_INVALID and "frame" in str(refused.value)
        image, _, info = frame.render()
        assert info["status"] == 0
        assert_bits_equal(image, before["pixels"], "the frame of the scene that refused the morph")
        frame.close()
        unchanged("after the live frame")
        g.morph(weights={0: other})
        assert_bits_equal(g.mesh_vertices(0), morph_ref.morph(meshes[0][0], targets, other), "a morph once the frame is gone")
        # unbinding, then morphing, is refused; the shape stays
        shape = g.mesh_vertices(0)
        g.bind_morphs(0, [])
        assert g.morphs(0) == (0, 0)
        with pytest.raises(binding.PtError) as refused:
            g.morph(weights={0: other})
        assert refused.value.code == PT_ERR_INVALID and "no morph set" in str(refused.value)
        assert_bits_equal(g.mesh_vertices(0), shape, "unbinding changes no geometry")
        g.bind_morphs(0, None)  # (unbinding twice is no fault)
        del rig
    finally:
        g.close()
        plain.close()
