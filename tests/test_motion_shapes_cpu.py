"""Motion for deformed meshes without a GPU (include/pt_motion_shapes.h): the numpy restatement
tests/motion_shapes_ref.py against tests/motion_ref.py's matrix route where a "deformation" is a rigid motion of the vertices, the
bending-card scenario of tests/test_gpu_motion_shapes.py run entirely through the restatements, and the header's place in the ABI."""
import ctypes as C
import os
import re

import numpy as np

from cpupathtrace_amd import binding, build, scenes
from tests import denoise_ref as dr
from tests import motion_ref, temporal_motion_ref, temporal_ref
from tests import motion_shapes_cases as cases
from tests import motion_shapes_ref as msr
from tests import test_gpu_pose as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# The largest absolute differences test_a_rigid_deformation_is_the_matrix_route measured between the per-vertex route and the matrix
# route (two fp32 evaluation orders of the same point): previous position 1.79e-07, previous normal 2.38e-07.  The test asserts 4 x that.
RIGID_POSITION, RIGID_NORMAL = 1.79e-07, 2.38e-07


def _flat(description, pos, nrm):
    n = len(pos)
    return motion_ref.flat_scene(description, pos, nrm, np.zeros(n, np.uint8), np.full(n, scenes.NO_MATERIAL, np.uint32))


def test_a_rigid_deformation_is_the_matrix_route(oracle_lib):
    """The patch, flat-shaded, under C; its vertices are turned and shifted in mesh space by R (computed in float32, as a caller would).
    Per vertex: marked = (V, C), current = (R V, C).  By matrices: the same hits with current = C R and previous = C through
    pt_motion_table.  Both describe where C V was; they differ by the rounding of two evaluation orders."""
    w, h = 32, 24
    cam = scenes.camera((0.0, 0.0, -0.9), (0.0, 0.0, 1.0), (0, 1, 0), 0.6, 1.0, -w / float(h))
    v, f = cases.patch()
    c = cases.place(-0.05, 0.05, 0.4, 0.9, degrees=10.0)
    r = cases.place(0.04, -0.03, -0.05, 1.0, degrees=-7.0)
    moved = (v @ r[:3, :3].T + r[:3, 3]).astype(F)
    description = tp._flat_scene(None, [], [])[0]
    n_desc = len(description["obj_kind"])
    pos, nrm = cases.assemble(c, moved, f)
    local = msr.kept_faces(c, moved, f)
    assert len(pos) == len(f) == 72
    flat = _flat(description, pos, nrm)
    first, count = [n_desc], [len(pos)]
    got, counts = msr.host_motion(oracle_lib, flat, cam, w, h, first, count, [msr.DEFORMED], None, None, pos, {0: (f, v, c, local)})
    current = (c.astype(np.float64) @ r.astype(np.float64)).astype(F)
    kind, back, normal = binding.motion_table(current[None], c[None])
    assert kind.tolist() == [motion_ref.MOVED]
    want, _ = motion_ref.host_motion(oracle_lib, flat, cam, w, h, first, count, kind, back, normal)
    assert counts["deformed"] >= 100 and counts["no previous"] == 0, counts
    on = got[..., 0, 3] > 0
    assert (got[..., :, 3] == want[..., :, 3]).all()
    assert not (got[..., 0, :3][on] == dr.host_features(oracle_lib, flat, cam, w, h)[..., 2, :3][on]).all()  # (it did move)
    d_pos = float(np.abs(got[..., 0, :3].astype(np.float64) - want[..., 0, :3]).max())
    d_nrm = float(np.abs(got[..., 1, :3].astype(np.float64) - want[..., 1, :3]).max())
    print("rigid deformation vs matrix route: largest difference of the previous position %.3g, of the previous normal %.3g" % (d_pos, d_nrm))
    assert d_pos <= 4 * RIGID_POSITION and d_nrm <= 4 * RIGID_NORMAL, (d_pos, d_nrm)


def test_the_bending_card_through_the_restatements(oracle_lib):
    """GPU test 7's scenario with every stage restated: the assembler (cases.assemble), the features (denoise_ref), the marked motion
    (motion_shapes_ref) and the push (temporal_motion_ref), so the inputs are known to satisfy its conditions before a GPU sees them.  At the GPU test's own 64 x 48, not at 32 x 24:
    the conditions carry test_a_sliding_card_keeps_its_history's absolute pixel counts (at least 100 pixels the card fills, 50 away from
    its silhouette), which a quarter of the pixels cannot meet (48 filled pixels were measured at 32 x 24), and the inputs a GPU sees are
    these."""
    w, h = cases.CARD_W, cases.CARD_H
    cam = cases.CARD_CAMERA
    v, f = cases.card()
    bowed = cases.card_bowed()
    assert float(-bowed[:, 2].min()) > 5.9 * cases.card_tolerance() > 0
    description = tp._flat_scene(None, [], [])[0]
    n_desc = len(description["obj_kind"])
    pos0, nrm0 = cases.assemble(cases.CARD_AT, v, f)
    pos1, nrm1 = cases.assemble(cases.CARD_AT, bowed, f)
    assert len(pos0) == len(pos1) == 128
    flat0, flat1 = _flat(description, pos0, nrm0), _flat(description, pos1, nrm1)
    f0, f1 = dr.host_features(oracle_lib, flat0, cam, w, h), dr.host_features(oracle_lib, flat1, cam, w, h)
    first, count = [n_desc], [128]
    on0, _ = motion_ref.host_motion(oracle_lib, flat0, cam, w, h, first, count, [motion_ref.NONE], None, None)
    local = msr.kept_faces(cases.CARD_AT, bowed, f)
    m1, counts = msr.host_motion(oracle_lib, flat1, cam, w, h, first, count, [msr.DEFORMED], None, None, pos1, {0: (f, v, cases.CARD_AT, local)})
    assert counts["deformed"] >= 20 and counts["no previous"] == 0, counts
    img = np.ones((h, w, 4), F)
    p = temporal_ref.params()
    marked, plain = temporal_ref.TemporalState(), temporal_ref.TemporalState()
    _, n0 = temporal_motion_ref.push(marked, img, f0, temporal_motion_ref.static_motion(f0), cam, p)
    temporal_motion_ref.push(plain, img, f0, temporal_motion_ref.static_motion(f0), cam, p)
    _, n_marked = temporal_motion_ref.push(marked, img, f1, m1, cam, p)
    _, n_plain = temporal_motion_ref.push(plain, img, f1, temporal_motion_ref.static_motion(f1), cam, p)
    cases.check_card(f0, on0, f1, m1, n0, n_marked, n_plain, w, h)


def test_symbols_are_exported_and_declared_in_their_own_header():
    build.build()
    lib = C.CDLL(binding.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pt_motion_shapes.h")).read()
    declared = set(re.findall(r"^int (pt_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(binding.MOTION_SHAPES_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    top = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert top.index('#include "pt_deform.h"') < top.index('#include "pt_motion_shapes.h"') and top.index('#include "pt_motion.h"') < top.index('#include "pt_motion_shapes.h"')
    fields = re.search(r"typedef struct pt_motion_mark_info \{(.*?)\} pt_motion_mark_info;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [decl.split()[-1] for decl in fields.split(";") if decl.strip()]
    assert names == [n for n, _ in binding.MotionMarkInfo._fields_]
    assert binding.MOTION_DEFORMED == 3 and "PT_MOTION_DEFORMED = 3" in header
    prose = re.sub(r"\s+", " ", header.replace("\n *", " "))
    assert "THE PREVIOUS NORMAL IS AN APPROXIMATION" in prose and "Left out: view batches" in prose


def test_refusals_come_before_any_device():
    lib = binding.load()
    err = lambda: lib.pt_last_error().decode()
    for call in (lambda: lib.pt_scene_motion_mark(None, None), lambda: lib.pt_scene_motion_unmark(None), lambda: lib.pt_scene_get_motion_mark(None, None, None),
                 lambda: lib.pt_scene_get_triangle_faces(None, None, None)):
        assert call() == 1 and "null scene" in err()  # PT_ERR_INVALID
    info = binding.MotionMarkInfo()
    info.n_instances = info.allocations = 7
    assert lib.pt_scene_motion_mark(None, C.byref(info)) == 1 and (info.n_instances, info.allocations) == (0, 0)  # (cleared whatever happens)


def test_cpp_program_compiles_and_links(tmp_path):
    """tests/cpp/motion_shapes_test.cpp (run by tests/test_gpu_motion_shapes.py) builds against the installed headers: Scene::markMotion
    and unmarkMotion are declared, and the class's data members are what they were."""
    from cpupathtrace_amd import build_host
    exe = str(tmp_path / "motion_shapes_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "motion_shapes_test.cpp")], exe, extra_flags=["-O1"])
    assert os.path.exists(exe)
    world = open(os.path.join(ROOT, "include", "PathTrace", "detail", "world.h")).read()
    assert "void markMotion();" in world and "void unmarkMotion();" in world
    assert "virtual void markMotion" not in world and "virtual void unmarkMotion" not in world
