"""Scenes from indexed meshes and instances, assembled on the device (include/pt_mesh.h, pt_mesh_batch.hip), bit for bit against io::loadMesh:
the golden answers of the compiled reference (tests/golden/mesh_assembly.npz) and the host library's loader (pth_load_mesh, which
test_oracle_vs_reference.py holds equal to the reference) for pt_mesh_assemble, and a flat pt_scene_create scene of the loader's triangles
for pt_scene_create_meshes: tree, emitters, hits, triangles and pixels.  No tolerance anywhere; NaN compares by NaN-ness."""
import ctypes as C
import os

import numpy as np
import pytest

from cpupathtrace_amd import build_host, scenes
from tests import mesh_cases
from tests.util import assert_bits_equal, env

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_assembly.npz")


@pytest.fixture(scope="module")
def host():
    return C.CDLL(build_host.build())


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _loaded(host, vertices, faces, matrix, smooth):
    return mesh_cases.load_mesh(host, "pth_", vertices, faces, matrix, smooth)


@pytest.mark.parametrize("mesh", list(mesh_cases.MESHES))
def test_assemble_matches_loader_and_golden(host, golden, mesh):
    from cpupathtrace_amd import binding
    v, f = mesh_cases.MESHES[mesh]
    assert_bits_equal(golden["vertices__" + mesh], v, "fixture vertices")
    assert_bits_equal(golden["faces__" + mesh], f, "fixture faces")
    answers = {}
    for transform, m in mesh_cases.TRANSFORMS.items():
        assert_bits_equal(golden["matrix__" + transform], m, "fixture matrix")
        for smooth in (0, 1):
            key = mesh_cases.case_key(mesh, transform, smooth)
            cap = len(f) + 3
            whole_p, out_p = mesh_cases.guarded(cap)
            whole_n, out_n = mesh_cases.guarded(cap)
            n, pos, nrm = binding.mesh_assemble(v, f, m, smooth, capacity=cap, out_pos=out_p, out_nrm=out_n)
            mesh_cases.assert_guards(whole_p, cap, n, key + ": positions written outside the result")
            mesh_cases.assert_guards(whole_n, cap, n, key + ": normals written outside the result")
            n_host, pos_host, nrm_host = _loaded(host, v, f, m, smooth)
            assert n == n_host == int(golden["count__" + key]), (key, n, n_host, int(golden["count__" + key]))
            assert_bits_equal(pos, pos_host, key + ": positions vs pth_load_mesh")
            assert_bits_equal(nrm, nrm_host, key + ": normals vs pth_load_mesh")
            assert_bits_equal(pos, golden["pos__" + key].view(F), key + ": positions vs the reference")
            assert_bits_equal(nrm, golden["nrm__" + key].view(F), key + ": normals vs the reference")
            answers[(transform, smooth)] = (n, pos.copy(), nrm.copy())
            if n > 1:
                # a capacity smaller than the result: the count comes back and nothing is written past the capacity
                small = n // 2
                whole_p, out_p = mesh_cases.guarded(small)
                whole_n, out_n = mesh_cases.guarded(small)
                n2, pos2, nrm2 = binding.mesh_assemble(v, f, m, smooth, capacity=small, out_pos=out_p, out_nrm=out_n)
                assert n2 == n and len(pos2) == small
                mesh_cases.assert_guards(whole_p, small, small, key + ": positions written past the capacity")
                mesh_cases.assert_guards(whole_n, small, small, key + ": normals written past the capacity")
                assert_bits_equal(pos2, pos[:small], key + ": positions, small capacity")
                assert_bits_equal(nrm2, nrm[:small], key + ": normals, small capacity")
    if mesh == "degenerate":
        for transform in ("identity", "scale_translate", "mirror", "flatten"):
            mesh_cases.share_conditions(answers[(transform, 0)][0])
        n, pos, _ = answers[("projective", 0)]
        assert 0 < n < answers[("identity", 0)][0] and np.isfinite(pos).all()  # the faces on w' = 0 vanish, what stays is finite
        assert answers[("tiny", 0)][0] == 0
        assert not np.isfinite(answers[("huge", 1)][2]).all()
    if mesh == "smoothing":
        mesh_cases.smoothing_conditions(v, f, answers[("identity", 0)][2], answers[("identity", 1)][2])


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------

IN_BOX = np.array(scenes.DRAGON_BOX_TRANSFORM, F)  # the bumpy sphere (radius 40 around (0, 50, 0)) into the unit box
SMALL_IN_BOX = np.array([[0.015, 0, 0, 0.1], [0, 0.02, 0, -0.1], [0, 0, 0.015, 0.2], [0, 0, 0, 1]], F)  # the +-40 families


def _base(sb):
    """The Box's walls and light quad, a sphere and a point light: both object kinds and both light kinds."""
    sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)))
    light = sb.material((1, 1, 1, 1), 1.0, (1, 1, 1, 1))
    sb.triangles(scenes.make_plane((-0.25, F(1.0) - F(0.01), -0.25), (0.25, F(1.0) - F(0.01), 0.25)), light)
    sb.sphere((0.55, -0.7, -0.3), 0.3, sb.material((0, 0, 1, 1), bsdf=scenes.BSDF_MIRROR))
    sb.point_light((-0.6, 0.7, -0.6), (0.5, 0.5, 0.4, 1.0))


CAMERA = scenes.camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0)


def _pair(host, instances, materials, desc_normals=True):
    """(mesh scene, flat scene, loader counts): `instances` are (vertices, faces, matrix, material name, cull, smooth); the flat scene
    has the loader's triangles appended in instance order with explicit normals."""
    a, b = scenes.SceneBuilder(), scenes.SceneBuilder()
    counts = []
    for sb in (a, b):
        _base(sb)
        mats = {name: sb.material(**kw) for name, kw in materials.items()}
        mats[None] = scenes.NO_MATERIAL
        for v, f, m, material, cull, smooth in instances:
            if sb is a:
                sb.mesh(v, f, m, mats[material], cull=cull, smooth=smooth)
            else:
                n, pos, nrm = _loaded(host, v, f, m, int(smooth))
                counts.append(n)
                sb.triangles(pos.reshape(-1, 3, 3), mats[material], cull=cull, normals=nrm.reshape(-1, 3, 3))
    sa, sb_ = a.build(), b.build()
    if not desc_normals:
        sa["tri_nrm"] = None  # the description's own triangles get their face normals on the device (or from the builder)
    return sa, sb_, counts


def _rays(n=4096, seed=5):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([rng.uniform(-0.95, 0.95, (n, 3)), d], axis=1).astype(F)


def _assert_same_scene(sa, sb_, counts, mode, spp=(4, 16), frame=True):
    from cpupathtrace_amd import binding
    with env(PT_BUILD=mode) if mode else env():
        ga, gb = binding.Scene(sa), binding.Scene(sb_)
        try:
            n_desc = len(sa["obj_kind"])
            first, count = ga.instance_ranges()
            assert count.tolist() == counts, (count.tolist(), counts)
            assert first.tolist() == (n_desc + np.concatenate([[0], np.cumsum(counts)[:-1]])).astype(np.int64).tolist()
            assert ga.n_objects == gb.n_objects == n_desc + sum(counts)
            assert ga.info() == gb.info()
            for x, y, what in zip(ga.bvh_dump(), gb.bvh_dump(), ("topology", "boxes")):
                assert_bits_equal(x, y, "BVH " + what)
            for x, y, what in zip(ga.emissive(), gb.emissive(), ("order", "CDF")):
                assert_bits_equal(x, y, "emitters: " + what)
            rays = _rays()
            (ta, oa), (tb, ob) = ga.get_intersection(rays), gb.get_intersection(rays)
            assert_bits_equal(ta, tb, "closest hit t")
            assert_bits_equal(oa, ob, "closest hit object")
            assert (oa >= n_desc).sum() > 100 or sum(counts) < 100  # the rays do meet the instances
            # the triangles the builder took: every triangle object of the description and of the instances
            n_tri_desc = len(sa["tri_pos"])  # (the description's triangles are its first objects, the sphere follows them: _base)
            for start, length, at in ((0, n_tri_desc, 0), (n_desc, sum(counts), n_tri_desc), (n_tri_desc - 2, 2, n_tri_desc - 2)):
                pos, nrm, cull, mat = ga.triangles(start, length)
                assert_bits_equal(pos, sb_["tri_pos"][at:at + length], "get_triangles positions")
                assert_bits_equal(nrm, sb_["tri_nrm"][at:at + length], "get_triangles normals")
                assert_bits_equal(cull, sb_["tri_cull"][at:at + length], "get_triangles cull")
                assert_bits_equal(mat, sb_["tri_material"][at:at + length], "get_triangles material")
            with pytest.raises(binding.PtError) as refused:
                ga.triangles(n_tri_desc - 1, 3)  # the sphere lies in this range
            assert refused.value.code == 1
            with pytest.raises(binding.PtError) as refused:
                gb.triangles(0, 1)  # a scene of plain pt_scene_create keeps no arrays
            assert refused.value.code == 4
            if frame:
                opt = scenes.options(64, 64, *spp)
                assert_bits_equal(ga.process_job(CAMERA, opt, base_seed=77), gb.process_job(CAMERA, opt, base_seed=77), "pixels")
        finally:
            ga.close()
            gb.close()


GLASS = {"glass": dict(diffuse=(1, 1, 1, 1), ior=1.5, bsdf=scenes.BSDF_GLASS)}


@pytest.mark.parametrize("smooth", [0, 1])
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("nu,nv", [(24, 16), (48, 24)])  # 720 triangles: the host builder by default; 2208: the device builder
def test_mesh_scene_equals_flat_scene(host, nu, nv, mode, smooth):
    v, f = scenes.bumpy_sphere_vertices(nu, nv)
    sa, sb_, counts = _pair(host, [(v, f, IN_BOX, "glass", False, bool(smooth))], GLASS, desc_normals=False)
    assert counts == [2 * nu * (nv - 1)]
    _assert_same_scene(sa, sb_, counts, mode)


@pytest.mark.parametrize("nu,nv", [(24, 16), (48, 24)])
def test_mesh_scene_default_builder(host, nu, nv):
    """No PT_BUILD: 720 triangles go to the host builder, 2208 to the device builder, by the number of objects AFTER rejection."""
    v, f = scenes.bumpy_sphere_vertices(nu, nv)
    sa, sb_, counts = _pair(host, [(v, f, IN_BOX, "glass", False, True)], GLASS)
    _assert_same_scene(sa, sb_, counts, None, spp=(4, 4))


def _shift(m, dx, dy, dz):
    out = np.array(m, F)
    out[:3, 3] += np.array([dx, dy, dz], F)
    return out


@pytest.mark.parametrize("variant", ["past_lds_table", "below_lds_table"])
def test_instances_share_a_mesh(host, variant):
    """One mesh under three instances with different transforms, materials (Lambertian, glass, emissive) and cull flags, a second mesh
    in between.  The emissive instance's triangles all register: 720 + 2 emitters (past PT_LDS_TABLE_MAX = 16, device builder), or
    8 + 2 (below it, host builder)."""
    from cpupathtrace_amd import binding
    nu, nv = (24, 16) if variant == "past_lds_table" else (4, 2)
    v, f = scenes.bumpy_sphere_vertices(nu, nv)
    v2, f2 = mesh_cases.MESHES["faces64"]
    half = np.array(IN_BOX, F)
    half[:3, :3] *= F(0.5)
    half[1, 3] = F(-0.25)
    materials = dict(GLASS, white=dict(diffuse=(0.8, 0.7, 0.6, 1.0)), lamp=dict(diffuse=(1, 1, 1, 1), emission=(1.0, 0.9, 0.8, 2.0)))
    instances = [(v, f, _shift(half, -0.5, -0.4, 0.2), "white", True, True),
                 (v2, f2, SMALL_IN_BOX, None, False, False),
                 (v, f, _shift(half, 0.3, 0.1, 0.4), "glass", False, True),
                 (v, f, _shift(half, -0.2, 0.5, -0.3), "lamp", True, False)]
    sa, sb_, counts = _pair(host, instances, materials)
    assert len(sa["meshes"]) == 2 and len(sa["instances"]) == 4
    n_tri = 2 * nu * (nv - 1)
    assert counts == [n_tri, 64, n_tri, n_tri]
    _assert_same_scene(sa, sb_, counts, None)
    g = binding.Scene(sa)
    try:
        assert g.info()["n_emissive"] == n_tri + 2
        assert (g.info()["n_emissive"] > 16) == (variant == "past_lds_table")
        obj, _ = g.emissive()
        first, count = g.instance_ranges()
        assert sorted(obj[obj >= first[3]].tolist()) == list(range(first[3], first[3] + count[3]))
    finally:
        g.close()


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("smooth", [0, 1])
def test_degenerate_mesh_as_a_scene(host, mode, smooth):
    """The ranges shrink by the dropped faces, and the objects the rays hit are the triangles pt_scene_get_triangles returns for them."""
    v, f = mesh_cases.MESHES["degenerate"]
    sa, sb_, counts = _pair(host, [(v, f, SMALL_IN_BOX, None, False, bool(smooth)), (v, f, _shift(SMALL_IN_BOX, -0.3, 0.2, -0.4), "glass", True, bool(smooth))], GLASS)
    mesh_cases.share_conditions(counts[0])
    assert counts[0] < len(f) and counts[1] < len(f)
    _assert_same_scene(sa, sb_, counts, mode, spp=(4, 4))


# ---- one creation call, one chain: what several instances of different kinds share ---------------------------------------------------------
# Every scene here is compared as created, never posed.

COLLAPSE = np.diag(np.array([0, 0, 0, 1], F))  # every vertex to the origin: every face is rejected (as tests/test_gpu_pose.py)


@pytest.mark.parametrize("mode", ["host", "device"])
def test_smooth_and_flat_instances_around_an_empty_one(host, mode):
    """A smooth instance, one whose every face is rejected, and a flat one in one call: the flat instance's corners take the key no vertex
    has, and the empty range lies between the two survivors."""
    from cpupathtrace_amd import binding
    v, f = scenes.bumpy_sphere_vertices(24, 16)
    v2, f2 = mesh_cases.MESHES["faces64"]
    instances = [(v, f, IN_BOX, "glass", False, True), (v2, f2, COLLAPSE, None, True, True), (v2, f2, SMALL_IN_BOX, None, False, False)]
    sa, sb_, counts = _pair(host, instances, GLASS)
    assert counts[0] > 0 and counts[1] == 0 and counts[2] > 0
    _assert_same_scene(sa, sb_, counts, mode, spp=(4, 4))
    with env(PT_BUILD=mode):
        g = binding.Scene(sa)
        try:
            first, count = g.instance_ranges()
            assert count.tolist() == counts and first[1] == first[2] == first[0] + counts[0]
        finally:
            g.close()


@pytest.mark.parametrize("mode", ["host", "device"])
def test_flat_instances_without_any_normals(host, mode):
    """No smooth instance and no normals in the description: there is no normal array at all, the builder makes every face normal."""
    v, f = scenes.bumpy_sphere_vertices(24, 16)
    v2, f2 = mesh_cases.MESHES["faces64"]
    instances = [(v, f, IN_BOX, "glass", False, False), (v2, f2, SMALL_IN_BOX, None, True, False), (v, f, _shift(IN_BOX, 0.2, 0.1, -0.2), None, False, False)]
    sa, sb_, counts = _pair(host, instances, GLASS, desc_normals=False)
    assert min(counts) > 0
    _assert_same_scene(sa, sb_, counts, mode, spp=(4, 4))


@pytest.mark.parametrize("mode", ["host", "device"])
def test_description_without_normals_and_a_smooth_instance(host, mode):
    """The description's triangles come without normals and one of two instances is smooth: the front of the normal array is filled with
    face normals on the device, the rest by the assembly."""
    v, f = scenes.bumpy_sphere_vertices(24, 16)
    v2, f2 = mesh_cases.MESHES["faces64"]
    instances = [(v2, f2, SMALL_IN_BOX, None, True, False), (v, f, IN_BOX, "glass", False, True)]
    sa, sb_, counts = _pair(host, instances, GLASS, desc_normals=False)
    assert min(counts) > 0
    _assert_same_scene(sa, sb_, counts, mode, spp=(4, 4))


@pytest.mark.parametrize("mode", ["host", "device"])
def test_eighteen_instances_in_one_creation(host, mode):
    """The nine meshes of the assembler's tests, flat and smooth, created in one call (the instances tests/test_gpu_pose.py poses): the
    triangles read back per instance range are the loader's."""
    from cpupathtrace_amd import binding
    from tests import pose_cases
    instances = [(v, f, _shift(SMALL_IN_BOX, 0.01 * i, 0, 0), None, False, bool(s)) for i, (v, f, s) in
                 enumerate((v, f, s) for v, f in pose_cases.MESH_LIST for s in (0, 1))]
    sa, sb_, counts = _pair(host, instances, GLASS)
    assert len(sa["instances"]) == 18 and len(sa["meshes"]) == 9
    _assert_same_scene(sa, sb_, counts, mode, frame=False)
    with env(PT_BUILD=mode):
        g = binding.Scene(sa)
        try:
            first, count = g.instance_ranges()
            assert count.tolist() == counts
            at = len(sa["tri_pos"])  # (the flat scene has the loader's triangles behind the description's, in instance order)
            for i, n in enumerate(counts):
                if n > 0:
                    pos, nrm, _, _ = g.triangles(int(first[i]), n)
                    assert_bits_equal(pos, sb_["tri_pos"][at:at + n], "instance %d: positions" % i)
                    assert_bits_equal(nrm, sb_["tri_nrm"][at:at + n], "instance %d: normals" % i)
                at += n
            assert at == len(sb_["tri_pos"])
        finally:
            g.close()
