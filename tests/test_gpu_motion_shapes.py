"""Motion for deformed meshes on the GPU (include/pt_motion_shapes.h): the features of the marked call are
pt_render_features' bit for bit; a mark alone changes nothing; mark + pose is pt_render_features_motion with the marked matrices; after a
deform or a morph the motion equals the oracle restatement tests/motion_shapes_ref.py bit for bit; the face table names the face every
triangle came from; refusals leave everything as it was; a card that bows toward the camera keeps its history; and
Scene.denoise_sequence_shapes(deforms=...) is the explicit loop.  The scene family: a 6 x 6-quad smooth patch used by two instances, an 8-face
flat mesh with two degenerate faces spliced in (so face_of is not the identity), the closed box of tests/test_gpu_motion.py, 32 x 24
frames, the tree once in LDS and once -- with a dense static sphere added -- in HBM.  The assembler never takes more than one chunk at
these sizes: only tests/test_face_table_cpu.py reaches the table over several chunks."""
import numpy as np
import pytest

from cpupathtrace_amd import binding, scenes
from tests import motion_ref
from tests import motion_shapes_cases as cases
from tests import motion_shapes_ref as msr
from tests import test_gpu_pose as tp
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 32, 24
CAMERA = scenes.camera((0.0, 0.0, -0.9), (0.0, 0.0, 1.0), (0, 1, 0), 0.6, 1.0, -W / float(H))
OPT = scenes.options(W, H, 4, 4)
PATCH, FLAT8 = cases.patch(), cases.flat8()
SPHERE = tp._sphere(48, 24)
AT = [cases.place(-0.42, 0.3, 0.45, 0.7), cases.place(0.42, 0.28, 0.55, 0.7, degrees=15.0), cases.place(0.0, -0.42, 0.3, 0.7), tp._shift(tp.IN_BOX, -0.6, -0.1, 0.4, 0.3)]
AT_B = [cases.place(-0.4, 0.33, 0.4, 0.72, degrees=-6.0), cases.place(0.4, 0.25, 0.5, 0.68, degrees=20.0)]
NAN = np.full((4, 4), np.nan, F)
MESH_OF = [0, 0, 1, 2]
ST, MV, NO, DF = motion_ref.STATIC, motion_ref.MOVED, motion_ref.NONE, msr.DEFORMED

# a rig of two bones over the patch's x, and two morph targets: one dense, one sparse
_x = PATCH[0][:, 0]
SKIN_BONES = np.tile(np.array([[0, 1]], np.uint32), (len(_x), 1))
SKIN_WEIGHTS = np.stack([0.5 - _x, 0.5 + _x], axis=1).astype(F)
BONES = np.stack([cases.place(0.02, 0.0, -0.05, 1.0, degrees=8.0)[:3], cases.place(-0.03, 0.04, 0.06, 0.95, degrees=-10.0)[:3]]).astype(F)
MORPHS = [(None, np.stack([np.zeros_like(_x), 0.05 * _x, 0.12 * PATCH[0][:, 1]], axis=1).astype(F)),
          (np.arange(0, 42, 2, dtype=np.uint32), np.tile(np.array([[0.05, 0.0, -0.04]], F), (21, 1)))]


def _instances(tree):
    out = [(PATCH[0], PATCH[1], "white", False, True), (PATCH[0], PATCH[1], "white", False, True), (FLAT8[0], FLAT8[1], None, False, False)]
    if tree == "hbm":
        out.append((SPHERE[0], SPHERE[1], "white", True, True))
    return out


def _mark(g, r):
    r["mark info"] = g.mark_motion()
    r["marked matrices"] = g.pose_transforms()
    r["marked vertices"] = {m: g.mesh_vertices(m) for m in sorted(set(MESH_OF[:g.n_instances]))}


def _vertices(g, r):
    g.deform(vertices={0: cases.patch_bent(0.15)})
    _mark(g, r)
    g.deform(vertices={0: cases.patch_bent(-0.2)})


def _bones_and_pose(g, r):
    g.bind_skin(0, SKIN_BONES, SKIN_WEIGHTS)
    _mark(g, r)
    g.deform(bones={0: BONES}, transforms=AT_B, instances=[0, 1])


def _morph(g, r):
    g.bind_morphs(0, MORPHS)
    _mark(g, r)
    g.morph(weights={0: [0.7, -0.4]})


def _morph_and_bones(g, r):
    g.bind_morphs(0, MORPHS)
    g.bind_skin(0, SKIN_BONES, SKIN_WEIGHTS)
    g.morph(weights={0: [0.3, 0.5]})
    _mark(g, r)
    g.morph(weights={0: [-0.5, 0.8]}, bones={0: BONES})


def _rest(g, r):
    g.deform(vertices={0: cases.patch_bent(0.2)})
    _mark(g, r)
    g.deform(rest=[0])


def _first(g, r):
    _mark(g, r)
    g.deform(vertices={0: cases.patch_bent(0.2)})


def _revive(g, r):
    _mark(g, r)
    g.deform(vertices={1: cases.flat8_revived()})


def _nan(g, r):
    g.pose([NAN], instances=[1])
    _mark(g, r)
    g.deform(vertices={0: cases.patch_bent(0.15)}, transforms=[AT[1]], instances=[1])


def _pose_only(g, r):
    _mark(g, r)
    g.pose([AT_B[0], cases.place(0.05, -0.4, 0.32, 0.7, degrees=5.0)], instances=[0, 2])


# name: (what it does, the kinds of the first three instances)
CASES = {"vertices": (_vertices, [DF, DF, ST]), "bones and pose": (_bones_and_pose, [DF, DF, ST]), "morph": (_morph, [DF, DF, ST]),
         "morph and bones": (_morph_and_bones, [DF, DF, ST]), "rest": (_rest, [DF, DF, ST]), "first deform": (_first, [DF, DF, ST]),
         "revive": (_revive, [ST, ST, DF]), "nan": (_nan, [DF, NO, ST]), "pose only": (_pose_only, [MV, ST, MV])}
DEFORMING = [name for name in CASES if name != "pose only"]
_cache = {}


def _run(name, tree):
    """Everything the device says about a case, asked once."""
    if (name, tree) in _cache:
        return _cache[(name, tree)]
    r = {}
    g = binding.Scene(tp._mesh_scene(_instances(tree), AT))
    try:
        CASES[name][0](g, r)
        r["matrices"] = g.pose_transforms()
        r["vertices"] = {m: g.mesh_vertices(m) for m in r["marked vertices"]}
        r["first"], r["count"] = g.instance_ranges()
        r["info"] = g.info()
        r["mark"], r["kinds"] = g.motion_mark()
        r["features"] = g.render_features(CAMERA, OPT)
        r["marked"] = g.render_features_motion_marked(CAMERA, OPT)
        r["by matrices"] = g.render_features_motion(CAMERA, OPT, previous=r["marked matrices"])
        r["faces"] = g.triangle_faces()
        description = tp._flat_scene(None, [], [])[0]
        r["n_desc"] = len(description["obj_kind"])
        r["triangles"] = g.triangles(r["n_desc"], int(r["count"].sum()))
        r["flat"] = motion_ref.flat_scene(description, *r["triangles"])
    finally:
        g.close()
    _cache[(name, tree)] = r
    return r


def _meshes():
    return {0: PATCH, 1: FLAT8, 2: SPHERE}


def _face_table(r):
    n = len(r["matrices"])
    return msr.face_table([(r["matrices"][i], r["vertices"][MESH_OF[i]], _meshes()[MESH_OF[i]][1]) for i in range(n)])


@pytest.mark.parametrize("tree", ["lds", "hbm"])
def test_the_tree_is_where_the_scenario_says(tree):
    nodes = _run("first deform", tree)["info"]["n_nodes"]
    assert (nodes < 2 * 1024) == (tree == "lds"), nodes


@pytest.mark.parametrize("tree", ["lds", "hbm"])
@pytest.mark.parametrize("name", list(CASES))
def test_features_are_unchanged_and_kinds_are_as_said(name, tree):
    r = _run(name, tree)
    assert_bits_equal(r["marked"][0], r["features"], "%s (%s): features of the marked call" % (name, tree))
    assert_bits_equal(r["mark"], r["marked matrices"], name + ": the marked matrices")
    assert r["kinds"][:3].tolist() == CASES[name][1] and (r["kinds"][3:] == ST).all(), (name, r["kinds"])


@pytest.mark.parametrize("tree", ["lds", "hbm"])
def test_a_mark_alone_changes_nothing(tree):
    g = binding.Scene(tp._mesh_scene(_instances(tree), AT))
    try:
        g.deform(vertices={0: cases.patch_bent(0.1)})
        before = g.process_job(CAMERA, OPT, base_seed=5)
        g.mark_motion()
        feat, motion = g.render_features_motion_marked(CAMERA, OPT)
        assert (g.motion_mark()[1] == ST).all()
        assert_bits_equal(g.process_job(CAMERA, OPT, base_seed=5), before, "process_job after a mark")
        assert_bits_equal(feat, g.render_features(CAMERA, OPT), "features after a mark")
    finally:
        g.close()
    assert_bits_equal(motion[..., 0, :3], feat[..., 2, :3], "mark, then nothing: previous position")
    assert_bits_equal(motion[..., 1, :3], feat[..., 1, :3], "mark, then nothing: previous normal")
    assert (motion[..., :, 3] == 0).all() and (feat[..., 0, 3] > 0).mean() > 0.5


@pytest.mark.parametrize("tree", ["lds", "hbm"])
def test_mark_then_pose_is_the_matrix_route(tree):
    r = _run("pose only", tree)
    assert_bits_equal(r["marked"][1], r["by matrices"][1], "mark + pose vs render_features_motion(previous = the marked matrices)")
    assert_bits_equal(r["marked"][0], r["by matrices"][0], "... and its features")
    assert (r["marked"][1][..., 0, 3] > 0).mean() >= 0.05


@pytest.mark.parametrize("tree", ["lds", "hbm"])
@pytest.mark.parametrize("name", DEFORMING)
def test_motion_equals_the_restatement(oracle_lib, name, tree):
    r = _run(name, tree)
    n = len(r["matrices"])
    face_of, face_first, counts = _face_table(r)
    assert counts == r["count"].tolist(), (counts, r["count"])
    kind = r["kinds"]
    _, back, normal = binding.motion_table(r["matrices"], r["marked matrices"])
    shapes, at = {}, 0
    for i in range(n):
        if kind[i] == DF:
            shapes[i] = (_meshes()[MESH_OF[i]][1], r["marked vertices"][MESH_OF[i]], r["marked matrices"][i], face_of[at:at + counts[i]].astype(np.int64) - face_first[i])
        at += counts[i]
    want, seen = msr.host_motion(oracle_lib, r["flat"], CAMERA, W, H, r["first"], r["count"], kind, back, normal, r["triangles"][0], shapes)
    print(name, tree, "kinds", kind.tolist(), "survivors", r["count"].tolist(), seen)
    assert seen["deformed"] >= 20, seen
    if name == "revive":
        assert seen["no previous"] >= 5, seen
    if name == "nan":
        assert seen["none"] >= 5, seen
    feat, motion = r["marked"]
    assert_bits_equal(motion, want, "%s (%s): marked motion vs the oracle restatement" % (name, tree))
    if name != "revive":
        assert not (motion == r["by matrices"][1]).all()  # (the matrices alone do not say it)


@pytest.mark.parametrize("tree", ["lds", "hbm"])
@pytest.mark.parametrize("name", ["pose only", "vertices", "morph", "revive"])
def test_triangle_faces_name_the_face_of_every_triangle(name, tree):
    r = _run(name, tree)
    face_of, face_first, counts = _face_table(r)
    assert r["faces"].dtype == np.uint32 and len(r["faces"]) == int(r["count"].sum())
    pos = r["triangles"][0].reshape(-1, 3, 3)
    at = 0
    for i in range(len(r["matrices"])):
        vertices, faces = r["vertices"][MESH_OF[i]], _meshes()[MESH_OF[i]][1]
        local = r["faces"][at:at + counts[i]].astype(np.int64) - face_first[i]
        assert ((local >= 0) & (local < len(faces))).all()
        corners = msr.transform(r["matrices"][i], vertices)[faces[local]]
        assert_bits_equal(pos[at:at + counts[i]], corners, "%s (%s): triangles of instance %d vs the corners of their faces" % (name, tree, i))
        at += counts[i]
    assert (r["faces"] == face_of).all()
    if name != "revive":
        flat = slice(int(r["count"][:2].sum()), int(r["count"][:3].sum()))
        assert len(r["faces"][flat]) == 8 and not (r["faces"][flat] - face_first[2] == np.arange(8)).all()  # (the spliced faces shift the others)


def test_refusals_leave_mark_table_and_output_as_they_were():
    sc, cam = scenes.box_scene()
    g = binding.Scene(sc)
    try:
        for call in (g.mark_motion, g.unmark_motion, g.triangle_faces, lambda: g.render_features_motion_marked(cam, OPT)):
            with pytest.raises(binding.PtError) as refused:
                call()
            assert refused.value.code == 4 and "has no instances" in str(refused.value)  # PT_ERR_UNSUPPORTED, in pt_deform.h's words
    finally:
        g.close()
    g = binding.Scene(tp._mesh_scene(_instances("lds"), AT))
    try:
        for call in (g.triangle_faces, g.motion_mark, lambda: g.render_features_motion_marked(CAMERA, OPT)):
            with pytest.raises(binding.PtError) as refused:
                call()
            assert refused.value.code == 1 and "no motion mark" in str(refused.value)  # PT_ERR_INVALID
        g.unmark_motion()  # (nothing to forget)
        g.mark_motion()
        with pytest.raises(binding.PtError) as refused:
            g.triangle_faces()
        assert refused.value.code == 1 and "no rebuild since the first mark" in str(refused.value)
        g.deform(vertices={0: cases.patch_bent(0.2)})
        mark, kinds, faces, out = g.motion_mark(), None, g.triangle_faces(), g.render_features_motion_marked(CAMERA, OPT)
        with pytest.raises(binding.PtError) as refused:
            g.deform(vertices={0: cases.patch_bent(0.3)[:-1]})
        assert refused.value.code == 1
        after = g.motion_mark()
        assert_bits_equal(after[0], mark[0], "the mark after a refused deform")
        assert (after[1] == mark[1]).all() and (g.triangle_faces() == faces).all()
        again = g.render_features_motion_marked(CAMERA, OPT)
        assert_bits_equal(again[1], out[1], "the marked motion after a refused deform")
        assert_bits_equal(again[0], out[0], "... and its features")
    finally:
        g.close()


def test_allocations_with_and_without_a_mark():
    """A mark allocates at the mark (two face tables, and the marked vertices of every deformed mesh), never in a rebuild; after unmark
    the scene counts what a scene that was never marked counts."""
    def deforms(g, amounts):
        return [g.deform(vertices={0: cases.patch_bent(a)}) for a in amounts]

    plain = binding.Scene(tp._mesh_scene(_instances("lds"), AT))
    marked = binding.Scene(tp._mesh_scene(_instances("lds"), AT))
    try:
        want = deforms(plain, (0.1, 0.2, 0.3, 0.4))
        first = deforms(marked, (0.1,))[0]
        at_mark = marked.mark_motion()
        assert at_mark["n_meshes_copied"] == 1 and at_mark["bytes_copied"] == 12 * len(PATCH[0])
        assert at_mark["allocations"] == first["allocations"] + 3  # the two tables and mesh 0's marked vertices
        while_marked = deforms(marked, (0.2, 0.3))
        assert marked.mark_motion()["allocations"] == at_mark["allocations"]  # (a second mark reuses everything)
        marked.unmark_motion()
        after = deforms(marked, (0.4,))[0]
        for info in while_marked + [after]:
            assert info["allocations"] == at_mark["allocations"], (info["allocations"], at_mark["allocations"])
        for a, b in zip(want, [first] + while_marked + [after]):
            assert (a["assembly_syncs"], a["assembly_chunks"], a["n_triangles"]) == (b["assembly_syncs"], b["assembly_chunks"], b["n_triangles"])
        assert [i["allocations"] for i in want] == [want[0]["allocations"]] * 4 == [first["allocations"]] * 4
        assert_bits_equal(marked.process_job(CAMERA, OPT, base_seed=3), plain.process_job(CAMERA, OPT, base_seed=3), "an unmarked scene renders what a never-marked one does")
    finally:
        plain.close()
        marked.close()


def test_a_bowing_card_keeps_its_history():
    """test_a_sliding_card_keeps_its_history's camera and box; the card is an 8 x 8 grid, flat at the mark, then bowed toward the camera
    by 6 position tolerances at its centre.  tests/test_motion_shapes_cpu.py holds the same scenario to the same conditions on the CPU."""
    w, h, cam = cases.CARD_W, cases.CARD_H, cases.CARD_CAMERA
    v, f = cases.card()
    opt = scenes.options(w, h, 4, 4)
    g = binding.Scene(tp._mesh_scene([(v, f, "white", False, False)], [cases.CARD_AT]))
    try:
        away = np.eye(4, dtype=F)
        away[:3, 3] = 5.0
        f0, on0 = g.render_features_motion(cam, opt, previous=[away])  # (a previous pose elsewhere marks the card's rays: motion[0].w)
        img0 = g.process_job(cam, opt, base_seed=1)
        g.mark_motion()
        g.deform(vertices={0: cases.card_bowed()})
        assert g.motion_mark()[1].tolist() == [DF]
        f1, m1 = g.render_features_motion_marked(cam, opt)
        img1 = g.process_job(cam, opt, base_seed=2)
    finally:
        g.close()
    with binding.TemporalDenoiser(w, h) as t, binding.TemporalDenoiser(w, h) as plain:
        _, n0 = t.denoise(img0, f0, cam)
        _, n_marked = t.denoise(img1, f1, cam, motion=m1)
        plain.denoise(img0, f0, cam)
        _, n_plain = plain.denoise(img1, f1, cam)
    cases.check_card(f0, on0, f1, m1, n0, n_marked, n_plain, w, h)


def test_denoise_sequence_shapes_is_the_explicit_loop():
    n = 3
    deforms = [{"vertices": {0: cases.patch_bent(0.1 * v)}, "transforms": [cases.place(-0.42 + 0.02 * v, 0.3, 0.45, 0.7)], "instances": [0]} for v in range(n)]
    morphs = [None, {"weights": {0: [0.4, 0.1]}}, None]  # (frame 1 morphs over its deform; frame 2 deforms again)
    frames, want = [], []
    g = binding.Scene(tp._mesh_scene(_instances("lds"), AT))
    try:
        g.bind_morphs(0, MORPHS)
        with binding.TemporalDenoiser(W, H) as t:
            for v in range(n):
                if v > 0:
                    g.mark_motion()
                g.deform(**deforms[v])
                if morphs[v]:
                    g.morph(**morphs[v])
                frames.append(g.process_job(CAMERA, OPT, base_seed=20 + v))
                feat, mot = g.render_features_motion_marked(CAMERA, OPT) if v > 0 else g.render_features_motion(CAMERA, OPT)
                assert v == 0 or (mot[..., 0, 3] > 0).mean() >= 0.05
                want.append(t.denoise(frames[v], feat, CAMERA, motion=mot)[0])
    finally:
        g.close()
    g = binding.Scene(tp._mesh_scene(_instances("lds"), AT))
    try:
        g.bind_morphs(0, MORPHS)
        got = g.denoise_sequence_shapes(frames, [CAMERA] * n, OPT, deforms=deforms, morphs=morphs)
        assert g.motion_mark()[1][:2].tolist() == [DF, DF]  # (left at the last frame, its predecessor marked)
    finally:
        g.close()
    assert_bits_equal(got, np.stack(want), "denoise_sequence_shapes(deforms=..., morphs=...) vs the explicit loop")


# ---- a bending object gains from its history ----------------------------------------------------------------------------------------------------

def _relmse(x, g, mask):
    x, g = x[..., :3].astype(np.float64)[mask], g[..., :3].astype(np.float64)[mask]
    return float(np.mean((x - g) ** 2 / (g ** 2 + 0.01)))


def test_a_bending_object_gains_from_its_history():
    """Modelled on test_a_moving_object_gains_from_its_history: Cornell box, static camera, 64 x 48, 16 spp, 8 pushes; a white bumpy
    sphere skinned to two bones (weights by height) whose upper bone turns by 4 degrees more per frame.  Only the ordering is asserted:
    on the pixels the object fills, relMSE against 1024 spp with the marked motion is below that of the plain push (DESIGN.md 4.11.2 has
    the measured values)."""
    import math
    w, h, n = 64, 48, 8
    sc, cam = scenes.cornell_scene(w, h)
    vertices, faces = scenes.bumpy_sphere_vertices(24, 16)
    base = tp._shift(tp.IN_BOX, 0.0, -0.3, -0.3, 0.6)
    sc = dict(sc, meshes=[(vertices, faces)], instances=[{"mesh": 0, "transform": base, "smooth": True, "cull": True, "material": scenes.NO_MATERIAL}])
    up = np.clip((vertices[:, 1] - 10.0) / 80.0, 0.0, 1.0).astype(F)  # the sphere has radius 40 around (0, 50, 0)
    bones, weights = np.tile(np.array([[0, 1]], np.uint32), (len(up), 1)), np.stack([1.0 - up, up], axis=1).astype(F)

    def rig(v):
        a = math.radians(4.0 * v)
        turn = np.eye(4)
        turn[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
        to, back = np.eye(4), np.eye(4)
        to[:3, 3], back[:3, 3] = (0.0, 10.0, 0.0), (0.0, -10.0, 0.0)  # about the sphere's foot
        return np.stack([np.eye(4)[:3], (to @ turn @ back)[:3]]).astype(F)

    opt = scenes.options(w, h, 16, 16)
    frames, feats, motions = [], [], []
    g = binding.Scene(sc)
    try:
        g.bind_skin(0, bones, weights)
        for v in range(n):
            if v > 0:
                g.mark_motion()
            g.deform(bones={0: rig(v)})
            frames.append(g.process_job(cam, opt, base_seed=1 + v))
            feat, motion = g.render_features_motion_marked(cam, opt) if v > 0 else g.render_features_motion(cam, opt)
            feats.append(feat)
            motions.append(motion)
        truth = g.process_job(cam, scenes.options(w, h, 1024, 1024), base_seed=99)
    finally:
        g.close()
    with binding.TemporalDenoiser(w, h) as t, binding.TemporalDenoiser(w, h) as plain:
        for v in range(n):
            out, hist = t.denoise(frames[v], feats[v], cam, motion=motions[v])
            out_plain, hist_plain = plain.denoise(frames[v], feats[v], cam)
    spatial = binding.denoise(frames[-1], feats[-1])
    obj = motions[-1][..., 0, 3] == 1
    assert obj.sum() >= 50, int(obj.sum())
    r_marked, r_plain = (_relmse(x, truth, obj) / _relmse(spatial, truth, obj) for x in (out, out_plain))
    print("%d object pixels: relMSE temporal / spatial with the marked motion %.3f, with the plain push %.3f; mean history %.2f against %.2f" % (
        obj.sum(), r_marked, r_plain, hist[obj].mean(), hist_plain[obj].mean()))
    assert r_marked < r_plain


# ---- the C++ layer ----------------------------------------------------------------------------------------------------------------------------

def test_cpp_follow_motion_across_deform(tmp_path):
    """tests/cpp/motion_shapes_test.cpp poses and deforms a Scene between the pushes of a TemporalDenoiser with follow_motion (which marks
    the scene after every push) and of one without: the first gives what the loop over the C ABI gives here on its frames -- mark, pose,
    deform, render_features_motion_marked, denoise(motion=...) --, the second the plain push, bit for bit.  (The pose-only C++ sequence,
    which takes the same marked route now, is held to its earlier output by tests/test_gpu_motion.py::test_cpp_follow_motion.)"""
    import os
    import subprocess
    from cpupathtrace_amd import build_host
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "motion_shapes_test")
    build_host.compile_program([os.path.join(root, "tests", "cpp", "motion_shapes_test.cpp")], exe, extra_flags=["-O1"])
    out_file = str(tmp_path / "frames.f32")
    path = [build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]
    r = subprocess.run([exe, out_file], env=dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(path)), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[ OK ]") == 5, r.stdout
    w, h = 40, 32
    frames, followed, plain = np.fromfile(out_file, np.float32).reshape(3, 3, h, w, 4)

    def shape(bow, lean):
        return np.array([[-0.25 + 0.3125 * i + (lean if j == 2 else 0.0), -0.25 + 0.25 * j, -bow if i == 1 else 0.0] for j in range(3) for i in range(3)], F)

    faces = np.array([f for j in range(2) for i in range(2) for f in ([3 * j + i, 3 * j + i + 4, 3 * j + i + 1], [3 * j + i, 3 * j + i + 3, 3 * j + i + 4])], np.int32)
    at = [np.eye(4, dtype=F), np.eye(4, dtype=F)]
    at[0][:3, 3], at[1][:3, 3] = (-0.125, 0.0, 0.5), (0.0, 0.0625, 0.5)
    sc, _ = scenes.box_scene()
    sc = dict(sc, meshes=[(shape(0.0, 0.0), faces)], instances=[{"mesh": 0, "transform": at[0], "smooth": False, "cull": False, "material": scenes.NO_MATERIAL}])
    cam = scenes.camera((0.0, 0.0, -0.875), (0.0, 0.0, 1.0), (0, 1, 0), 0.625, 1.0, -1.25)
    opt = scenes.options(w, h, 8, 8)
    g = binding.Scene(sc)
    try:
        with binding.TemporalDenoiser(w, h) as t, binding.TemporalDenoiser(w, h) as p:
            for v in range(3):
                if v > 0:
                    g.mark_motion()
                if v == 1:
                    g.pose([at[1]])
                    g.deform(vertices={0: shape(0.125, 0.0)})
                if v == 2:
                    g.deform(vertices={0: shape(0.1875, 0.0625)})
                feat, mot = g.render_features_motion_marked(cam, opt) if v > 0 else g.render_features_motion(cam, opt)
                if v > 0:
                    assert g.motion_mark()[1].tolist() == [DF] and (mot[..., 0, 3] > 0).mean() >= 0.02
                assert_bits_equal(t.denoise(frames[v], feat, cam, motion=mot)[0], followed[v], "C++ follow_motion across Scene::deform = the C-ABI loop, frame %d" % v)
                assert_bits_equal(p.denoise(frames[v], g.render_features(cam, opt), cam)[0], plain[v], "C++ without follow_motion = the plain push, frame %d" % v)
    finally:
        g.close()
    assert not (followed[1] == plain[1]).all()
