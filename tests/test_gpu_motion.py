"""Motion-aware temporal denoising on the GPU (include/pt_motion.h): the features of pt_render_features_motion are
pt_render_features' bit for bit, its motion is the features' position and normal where nothing moved and the oracle restatement
tests/motion_ref.py bit for bit where instances did, the motion push equals tests/temporal_motion_ref.py (history lengths exactly), a
motion in which nothing moved is the plain push bit for bit, a card that slides in its plane keeps its history, and
Scene.denoise_sequence(poses=...) is the explicit loop."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from cpupathtrace_amd import binding, scenes
from tests import motion_ref, pose_cases, temporal_motion_ref, temporal_ref
from tests import test_gpu_pose as tp
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NON_DEFAULT = {"spatial": {"iterations": 2, "sigma_luminance": 8.0}, "alpha_color": 0.5, "alpha_moments": 0.3, "max_history": 3,
               "moments_min_history": 2, "sigma_luminance_temporal": 8.0, "normal_min": 0.8, "position_tolerance": 1.0}  # tests/test_gpu_temporal.py's


def _roty(degrees):
    a = math.radians(degrees)
    m = np.eye(4, dtype=F)
    m[0, 0] = m[2, 2] = math.cos(a)
    m[0, 2], m[2, 0] = math.sin(a), -math.sin(a)
    return m


S = tp._shift
# the four instances of tests/test_gpu_pose.py (two bumpy spheres, faces64, the degenerate mesh), small enough to leave the walls and the
# mirror sphere in view of a camera inside the box; at B the third has no survivors (it lies between two that have)
POSE_A = [S(tp.IN_BOX, -0.55, 0.35, 0.5, 0.3), S(tp.IN_BOX, 0.1, 0.45, 0.55, 0.3), S(tp.SMALL_IN_BOX, -0.5, -0.3, 0.3), S(tp.SMALL_IN_BOX, 0.1, -0.2, 0.5)]
POSE_B = [(_roty(10) @ S(tp.IN_BOX, -0.45, 0.3, 0.45, 0.32)).astype(F), (_roty(-8) @ S(tp.IN_BOX, 0.2, 0.4, 0.5, 0.28)).astype(F), tp.COLLAPSE,
          (_roty(5) @ S(tp.SMALL_IN_BOX, 0.05, -0.25, 0.45)).astype(F)]
POSE_SUB = POSE_A[:3] + [POSE_B[3]]  # one instance moved, the others where they were
NAN = np.full((4, 4), np.nan, F)
PREVIOUS_NONE = [POSE_A[0], POSE_A[1], NAN, (POSE_A[3] @ tp.PROJECTIVE).astype(F)]  # "was not there", and a projective previous matrix
INSIDE = scenes.camera((-0.1, 0.0, -0.95), (0.2, -0.25, 0.3), (0, 1, 0), 0.6, 1.0, -64 / 48.0)
# the crossing pose of test_pose_across_builder_lds_and_emitter_thresholds: 2928 instance triangles, the tree in HBM
CROSS_B = [S(tp.IN_BOX, -0.3, -0.2, 0.2, 0.6), S(tp.IN_BOX, 0.4, 0.3, -0.1, 0.4)]
CROSS_A = [(_roty(-6) @ S(tp.IN_BOX, -0.35, -0.15, 0.25, 0.55)).astype(F), S(tp.IN_BOX, 0.45, 0.3, -0.05, 0.4)]
FEW_A = [POSE_A[2], POSE_A[3], S(tp.SMALL_IN_BOX, 0.3, 0.4, 0.6)]
FEW_B = [(_roty(-12) @ S(tp.SMALL_IN_BOX, -0.4, -0.35, 0.25)).astype(F), POSE_A[3], tp.COLLAPSE]

# name: (instances, created at, posed to = current, previous, camera, (w, h), the shares that must be >= 5 % of the hit rays)
SCENARIOS = {
    "A to B": ("four", POSE_A, POSE_B, POSE_A, INSIDE, (64, 48), ("description", "sphere", "moved")),
    "B to A": ("four", POSE_B, POSE_A, POSE_B, INSIDE, (61, 47), ("description", "sphere", "moved", "none")),
    "one of four": ("four", POSE_A, POSE_SUB, POSE_A, INSIDE, (64, 48), ("description", "sphere", "moved", "static")),
    "no previous": ("four", POSE_B, POSE_A, PREVIOUS_NONE, INSIDE, (61, 47), ("description", "sphere", "none")),
    "crossing": ("two lamps", [tp.COLLAPSE, tp.COLLAPSE], CROSS_B, CROSS_A, INSIDE, (61, 47), ("description", "moved")),
    # few enough objects for the tree to be served from LDS
    "few": ("few", FEW_A, FEW_B, FEW_A, INSIDE, (61, 47), ("description", "sphere", "moved", "static")),
}


def _instances(which):
    if which == "four":
        return tp._four_instances()[0]
    if which == "few":
        four = tp._four_instances()[0]
        return [four[2], four[3], four[2]]
    (v1, f1), (v2, f2) = tp._sphere(48, 24), tp._sphere(24, 16)
    return [(v1, f1, "lamp", False, True), (v2, f2, "lamp", True, False)]


_cache = {}


def _run(name):
    """Everything the device says about a scenario, asked once: the plain features, (features, motion) for previous = None, = the current
    pose and = the scenario's previous pose, the instance ranges and the flat scene of the triangles read back."""
    if name in _cache:
        return _cache[name]
    which, created, current, previous, cam, (w, h), _ = SCENARIOS[name]
    instances = _instances(which)
    opt = scenes.options(w, h, 4, 4)
    g = binding.Scene(tp._mesh_scene(instances, created))
    try:
        g.pose(current)
        first, count = g.instance_ranges()
        out = {"first": first, "count": count, "features": g.render_features(cam, opt), "info": g.info()}
        out["none"] = g.render_features_motion(cam, opt)
        out["same"] = g.render_features_motion(cam, opt, previous=current)
        out["previous"] = g.render_features_motion(cam, opt, previous=previous)
        out["features after"] = g.render_features(cam, opt)
        description = tp._flat_scene(None, [], [])[0]
        n_desc = len(description["obj_kind"])
        assert first[0] == n_desc
        out["flat"] = motion_ref.flat_scene(description, *g.triangles(n_desc, int(count.sum())))
    finally:
        g.close()
    _cache[name] = out
    return out


def test_poses_leave_an_instance_without_survivors_between_two_that_have():
    assert pose_cases.has_empty_between_survivors(_run("A to B")["count"].tolist())
    assert (_run("B to A")["count"] > 0).all()
    cross = _run("crossing")
    assert cross["count"].tolist() == [2208, 720] and cross["info"]["n_nodes"] >= 2 * 1024  # (the tree does not fit the LDS route)
    few = _run("few")
    assert few["count"].tolist()[2] == 0 and few["info"]["n_nodes"] < 2 * 1024  # ... and this one does


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_features_are_unchanged(name):
    r = _run(name)
    for which in ("none", "same", "previous"):
        assert_bits_equal(r[which][0], r["features"], "%s, previous = %s: features" % (name, which))
    assert_bits_equal(r["features after"], r["features"], name + ": pt_render_features after the motion passes")


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_static_identity(name):
    r = _run(name)
    for which in ("none", "same"):
        feat, motion = r[which]
        assert_bits_equal(motion[..., 0, :3], feat[..., 2, :3], "%s, previous = %s: previous position" % (name, which))
        assert_bits_equal(motion[..., 1, :3], feat[..., 1, :3], "%s, previous = %s: previous normal" % (name, which))
        assert (motion[..., 0, 3] == 0).all() and (motion[..., 1, 3] == 0).all()
        assert (feat[..., 0, 3] > 0).mean() > 0.5


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_motion_equals_the_restatement(oracle_lib, name):
    _, _, current, previous, cam, (w, h), shares = SCENARIOS[name]
    r = _run(name)
    kind, back, normal = binding.motion_table(np.array(current, F), np.array(previous, F))
    want, counts = motion_ref.host_motion(oracle_lib, r["flat"], cam, w, h, r["first"], r["count"], kind, back, normal)
    print(name, "kinds", kind.tolist(), "survivors", r["count"].tolist(), {k: round(v / counts["hit"], 3) for k, v in counts.items()})
    for share in shares:
        assert counts[share] >= 0.05 * counts["hit"], (name, share, counts)
    feat, motion = r["previous"]
    assert_bits_equal(motion, want, name + ": motion vs the oracle restatement")
    moved = motion[..., 0, 3] > 0
    assert moved.any() and not (motion[..., 0, :3][moved] == feat[..., 2, :3][moved]).all()


def test_a_scene_without_instances():
    sc, cam = scenes.box_scene()
    opt = scenes.options(61, 47, 4, 4)
    g = binding.Scene(sc)
    try:
        feat, motion = g.render_features_motion(cam, opt)
        assert_bits_equal(feat, g.render_features(cam, opt), "features of a scene without instances")
        assert_bits_equal(motion[..., 0, :3], feat[..., 2, :3], "its motion")
        assert (motion[..., :, 3] == 0).all()
        with pytest.raises(binding.PtError) as refused:
            g.render_features_motion(cam, opt, previous=np.eye(4, dtype=F)[None])
        assert refused.value.code == 4  # PT_ERR_UNSUPPORTED
    finally:
        g.close()


# ---- the push ----------------------------------------------------------------------------------------------------------------------------------

def _orbit(cam, degrees):
    o, la = np.asarray(cam["origin"], np.float64), np.asarray(cam["look_at"], np.float64)
    a = math.radians(degrees)
    d = o - la
    rot = np.array([d[0] * math.cos(a) + d[2] * math.sin(a), d[1], -d[0] * math.sin(a) + d[2] * math.cos(a)])
    return dict(cam, origin=tuple(float(v) for v in la + rot))


def _pose_of_frame(v, appearing=False):
    pose = [(_roty(3.0 * v) @ S(m, 0.02 * v, 0.0, 0.01 * v)).astype(F) for m in POSE_A]
    if appearing and v < 2:
        pose[2] = tp.COLLAPSE
    return pose


def _sequence(kind, n=5, w=64, h=48, spp=4):
    """n frames of the four instances moving: (cameras, frames, features, motions, poses); `appearing`: the third instance is not there in
    the first two frames and gets a NaN previous matrix in the third."""
    cams = [_orbit(INSIDE, 0.7 * v) if kind == "orbit" else INSIDE for v in range(n)]
    poses = [_pose_of_frame(v, kind == "appearing") for v in range(n)]
    opt = scenes.options(w, h, spp, spp)
    frames, feats, motions = [], [], []
    g = binding.Scene(tp._mesh_scene(tp._four_instances()[0], poses[0]))
    try:
        for v in range(n):
            previous = None
            if v > 0:
                g.pose(poses[v])
                previous = list(poses[v - 1])
                if kind == "appearing" and v == 2:
                    previous[2] = NAN
            frames.append(g.process_job(cams[v], opt, base_seed=11 + v))
            feat, motion = g.render_features_motion(cams[v], opt, previous=previous)
            feats.append(feat)
            motions.append(motion)
    finally:
        g.close()
    return cams, frames, feats, motions, poses


@pytest.mark.parametrize("kind", ["static", "orbit", "appearing"])
def test_push_equals_the_restatement(kind):
    w, h = 64, 48
    cams, frames, feats, motions, _ = _sequence(kind)
    assert all((m[..., 0, 3] > 0).mean() >= 0.05 for m in motions[1:])
    if kind == "appearing":
        assert (motions[2][..., 1, 3] > 0).mean() >= 0.02 and not (motions[3][..., 1, 3] > 0).any()
    for params in (None, NON_DEFAULT):
        p = temporal_ref.params(**(params or {}))
        state = temporal_ref.TemporalState()
        with binding.TemporalDenoiser(w, h, params=params) as t:
            for v, c in enumerate(cams):
                got, n = t.denoise(frames[v], feats[v], c, motion=motions[v])
                want, wn = temporal_motion_ref.push(state, frames[v], feats[v], motions[v], c, p)
                moved = motions[v][..., 0, 3] > 0
                print("%s frame %d: n in %s, on moved pixels %s; largest difference %.3g" % (
                    kind, v, np.unique(n), np.unique(n[moved]), np.abs(got.astype(np.float64) - want).max()))
                assert (n == wn).all(), "%s frame %d: %d history lengths differ" % (kind, v, int((n != wn).sum()))
                np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)
                if v > 0:
                    assert (n[moved] > 1).any()  # (history did follow the instances)


STATIC_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding, scenes
w, h = 61, 47
sc, cam = scenes.cornell_scene(w, h)
cams = [dict(cam, origin=(0.03 * k, 0.0, -3.0), look_at=(0.03 * k, 0.0, 0.0)) for k in range(4)]
gpu = binding.Scene(sc, device=0)
opt = scenes.options(w, h, 8, 8)
frames = gpu.process_views(cams, opt, base_seeds=[5, 6, 7, 8])
pairs = [gpu.render_features_motion(c, opt) for c in cams]
stream = torch.cuda.current_stream(0).cuda_stream
outs = {}
for form in ("plain", "host none", "host static", "device none", "device static"):
    t = binding.TemporalDenoiser(w, h)
    res = []
    for v in range(4):
        feat, motion = pairs[v]
        if form == "plain":
            res.append(t.denoise(frames[v], feat, cams[v]))
        elif form.startswith("host"):
            res.append(t.denoise(frames[v], feat, cams[v], motion=motion if form == "host static" else None))
        else:
            d_img, d_feat, d_mot = (torch.from_numpy(a).to("cuda:0") for a in (frames[v], feat, motion))
            d_out = torch.empty_like(d_img)
            d_n = torch.full((h, w), -5, dtype=torch.int32, device="cuda:0")
            t.denoise_device(d_img.data_ptr(), d_feat.data_ptr(), cams[v], d_out.data_ptr(), d_n.data_ptr(), stream,
                             motion=d_mot.data_ptr() if form == "device static" else None)
            res.append((d_out.cpu().numpy(), d_n.cpu().numpy()))
    t.close()
    outs[form] = res
ok = max(int(n.max()) for _, n in outs["plain"]) >= 4
for form in outs:
    same = all((a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1] == b[1]).all() for a, b in zip(outs[form], outs["plain"]))
    print("%s: %s" % (form, "bit-identical" if same else "DIFFERENT"))
    ok = ok and same
sys.exit(0 if ok else 1)
"""


def test_static_motion_is_the_plain_push():
    """Over a pan of the Cornell box: denoise(..., motion=None) and motion = the all-static motion of pt_render_features_motion equal
    TemporalDenoiser.denoise bit for bit, frames and history, host and device forms.  In a fresh interpreter in which torch opens the
    device first, as tests/test_gpu_temporal.py's."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", STATIC_CHILD, ROOT], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("bit-identical") == 5, r.stdout


# ---- a card that slides ----------------------------------------------------------------------------------------------------------------------

def _dilate(mask):
    out = mask.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            shifted = np.zeros_like(mask)
            ys, xs = slice(max(dy, 0), mask.shape[0] + min(dy, 0)), slice(max(dx, 0), mask.shape[1] + min(dx, 0))
            yd, xd = slice(max(-dy, 0), mask.shape[0] + min(-dy, 0)), slice(max(-dx, 0), mask.shape[1] + min(-dx, 0))
            shifted[yd, xd] = mask[ys, xs]
            out |= shifted
    return out


@pytest.mark.parametrize("m", [1, 3])
def test_a_sliding_card_keeps_its_history(m):
    """A flat quad 0.5 in front of the box's back wall, facing a static camera, slides in its own plane by m pixel footprints."""
    w, h = 64, 48
    cam = scenes.camera((0.0, 0.0, -0.9), (0.0, 0.0, 1.0), (0, 1, 0), 0.6, 1.0, -w / float(h))
    vertices = np.array([[-0.31, -0.27, 0.0], [0.33, -0.27, 0.0], [0.33, 0.29, 0.0], [-0.31, 0.29, 0.0]], F)
    faces = np.array([[0, 2, 1], [0, 3, 2]], np.int32)
    step = m * (1.4 * temporal_ref.footprint(cam, h))  # the card is 1.4 from the camera
    at = [np.eye(4, dtype=F), np.eye(4, dtype=F)]
    at[0][:3, 3] = (-0.05, 0.02, 0.5)
    at[1][:3, 3] = (-0.05 + step, 0.02, 0.5)
    opt = scenes.options(w, h, 4, 4)
    g = binding.Scene(tp._mesh_scene([(vertices, faces, "white", False, False)], at[:1]))
    try:
        away = np.eye(4, dtype=F)
        away[:3, 3] = 5.0
        f0, on0 = g.render_features_motion(cam, opt, previous=[away])  # (a previous pose elsewhere marks the card's rays: motion[0].w)
        img0 = g.process_job(cam, opt, base_seed=1)
        g.pose(at[1:])
        f1, m1 = g.render_features_motion(cam, opt, previous=at[:1])
        img1 = g.process_job(cam, opt, base_seed=2)
    finally:
        g.close()
    # (inside the closed box every ray hits, but for those that slip through the seam of two triangles: such pixels are left out)
    whole = (f0[..., 0, 3] == 1) & (f1[..., 0, 3] == 1)
    assert whole.mean() >= 0.97
    on1 = m1
    full0, full1, any0, any1 = on0[..., 0, 3] == 1, on1[..., 0, 3] == 1, on0[..., 0, 3] > 0, on1[..., 0, 3] > 0
    near = _dilate(any0 & ~full0) | _dilate(any1 & ~full1)  # within one pixel of the card's silhouette in either frame
    assert full1.sum() >= 100 and near.mean() < 0.15, (int(full1.sum()), float(near.mean()))
    with binding.TemporalDenoiser(w, h) as t:
        _, n0 = t.denoise(img0, f0, cam)
        _, n = t.denoise(img1, f1, cam, motion=m1)
    assert (n0 == 1).all()
    card = full0 & full1 & ~near & whole
    uncovered = full0 & ~any1 & whole
    # (a ray along the edge two walls share may report either of them, and the pose rebuilt the tree: the few pixels whose own wall
    # features changed between the frames are counted and left out)
    ties = ~any0 & ~any1 & ~(f0 == f1).all(axis=(-1, -2))
    assert ties.sum() <= 0.01 * w * h
    wall = ~any0 & ~any1 & ~near & whole & ~ties
    print("m = %d: %d card pixels, %d uncovered, %d wall, %d near the silhouette (%.1f %%)" % (m, card.sum(), uncovered.sum(), wall.sum(), near.sum(), 100 * near.mean()))
    assert card.sum() >= 50 and (n[card] == 2).all(), np.unique(n[card], return_counts=True)
    assert (n[full1 & ~near & whole] == 2).all()  # ... and so has every pixel the card fills now, away from its silhouette
    assert (n[uncovered] == 1).all()  # the wall behind is 0.5 away: more than position_tolerance footprints
    assert uncovered.sum() >= (m - 1) * 10
    assert wall.sum() >= 0.5 * w * h and (n[wall] == 2).all()


# ---- the upper layers ---------------------------------------------------------------------------------------------------------------------------

def test_denoise_sequence_with_poses_is_the_explicit_loop():
    w, h = 61, 47
    cams, frames, feats, motions, poses = _sequence("static", n=3, w=w, h=h)
    opt = scenes.options(w, h, 4, 4)
    want = []
    with binding.TemporalDenoiser(w, h) as t:
        for v in range(3):
            want.append(t.denoise(frames[v], feats[v], cams[v], motion=motions[v])[0])
    g = binding.Scene(tp._mesh_scene(tp._four_instances()[0], poses[2]))  # (created elsewhere: the sequence poses it)
    try:
        got = g.denoise_sequence(frames, cams, opt, poses=poses)
        assert_bits_equal(g.pose_transforms(), np.array(poses[2], F), "the scene is left at the last pose")
        plain = g.denoise_sequence(frames[2:], cams[2:], opt)
    finally:
        g.close()
    assert_bits_equal(got, np.stack(want), "denoise_sequence(poses=...) vs the explicit loop")
    assert_bits_equal(plain[0], binding.denoise(frames[2], feats[2]), "denoise_sequence without poses: a first push")


def test_cpp_follow_motion(tmp_path):
    """tests/cpp/motion_test.cpp poses a Scene between the pushes of a TemporalDenoiser with follow_motion and of one without: the first
    gives what render_features_motion + denoise(motion=...) give here on its frames, the second today's outputs, bit for bit."""
    from cpupathtrace_amd import build_host
    exe = str(tmp_path / "motion_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "motion_test.cpp")], exe, extra_flags=["-O1"])
    out_file = str(tmp_path / "frames.f32")
    path = [build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]
    r = subprocess.run([exe, out_file], env=dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(path)), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[ OK ]") == 4, r.stdout
    w, h = 40, 32
    frames, followed, plain = np.fromfile(out_file, np.float32).reshape(3, 3, h, w, 4)
    sc, _ = scenes.box_scene()
    vertices = np.array([[-0.25, -0.25, 0], [0.375, -0.25, 0], [0.375, 0.25, 0], [-0.25, 0.25, 0]], F)
    faces = np.array([[0, 2, 1], [0, 3, 2]], np.int32)
    poses = []
    for x, y, z in ((-0.125, 0.0, 0.5), (0.0, 0.0625, 0.5), (0.125, 0.0625, 0.375)):
        m = np.eye(4, dtype=F)
        m[:3, 3] = (x, y, z)
        poses.append([m])
    sc = dict(sc, meshes=[(vertices, faces)], instances=[{"mesh": 0, "transform": poses[0][0], "smooth": False, "cull": False, "material": scenes.NO_MATERIAL}])
    cam = scenes.camera((0.0, 0.0, -0.875), (0.0, 0.0, 1.0), (0, 1, 0), 0.625, 1.0, -1.25)
    opt = scenes.options(w, h, 8, 8)
    g = binding.Scene(sc)
    try:
        assert_bits_equal(g.denoise_sequence(frames, [cam] * 3, opt, poses=poses), followed, "C++ follow_motion = Scene.denoise_sequence(poses=...)")
        feats = []
        for v in range(3):
            g.pose(poses[v])
            feats.append(g.render_features(cam, opt))
    finally:
        g.close()
    with binding.TemporalDenoiser(w, h) as t:
        for v in range(3):
            assert_bits_equal(t.denoise(frames[v], feats[v], cam)[0], plain[v], "C++ without follow_motion = the plain push, frame %d" % v)
    assert not (followed[1] == plain[1]).all()


# ---- a moving object gains from its history ---------------------------------------------------------------------------------------------------

def _relmse(x, g, mask):
    x, g = x[..., :3].astype(np.float64)[mask], g[..., :3].astype(np.float64)[mask]
    return float(np.mean((x - g) ** 2 / (g ** 2 + 0.01)))


def test_a_moving_object_gains_from_its_history():
    """Cornell box, static camera, 128 x 128, 16 spp, 8 pushes; a white Lambertian bumpy sphere moves by about 2 pixel footprints and
    turns by 3 degrees per frame.  relMSE of the 8th output against 1024 spp at the 8th pose (DESIGN.md 4.11.1 has the measured values):
    on the pixels the object fills, the motion push must beat the spatial filter; on the static pixels it must be no worse than the plain
    push on the same frames (5 % margin for the different taps at the object's border)."""
    w = h = 128
    sc, cam = scenes.cornell_scene(w, h)
    vertices, faces = scenes.bumpy_sphere_vertices(24, 16)
    base = S(tp.IN_BOX, 0.0, -0.3, -0.3, 0.6)
    centre = (base.astype(np.float64) @ np.array([0.0, 50.0, 0.0, 1.0]))[:3]
    step = 2.0 * 2.7 * float(temporal_ref.footprint(cam, h))  # the object is about 2.7 from the camera

    def pose(v):
        there, back = np.eye(4), np.eye(4)
        there[:3, 3] = centre + np.array([step * (v - 3.5), 0.0, 0.0])
        back[:3, 3] = -centre
        return [(there @ _roty(3.0 * v).astype(np.float64) @ back @ base.astype(np.float64)).astype(F)]

    poses = [pose(v) for v in range(8)]
    sc = dict(sc, meshes=[(vertices, faces)], instances=[{"mesh": 0, "transform": poses[0][0], "smooth": True, "cull": True, "material": scenes.NO_MATERIAL}])
    opt = scenes.options(w, h, 16, 16)
    frames, feats, motions = [], [], []
    g = binding.Scene(sc)
    try:
        for v in range(8):
            if v > 0:
                g.pose(poses[v])
            frames.append(g.process_job(cam, opt, base_seed=1 + v))
            feat, motion = g.render_features_motion(cam, opt, previous=poses[v - 1] if v > 0 else None)
            feats.append(feat)
            motions.append(motion)
        truth = g.process_job(cam, scenes.options(w, h, 1024, 1024), base_seed=99)
    finally:
        g.close()
    with binding.TemporalDenoiser(w, h) as t, binding.TemporalDenoiser(w, h) as plain:
        for v in range(8):
            out, n = t.denoise(frames[v], feats[v], cam, motion=motions[v])
            out_plain, n_plain = plain.denoise(frames[v], feats[v], cam)
    spatial = binding.denoise(frames[7], feats[7])
    obj = motions[7][..., 0, 3] == 1
    static = (motions[7][..., 0, 3] == 0) & (feats[7][..., 0, 3] > 0)
    assert obj.sum() >= 200 and static.sum() >= 0.8 * w * h
    r_obj, r_obj_plain = (_relmse(x, truth, obj) / _relmse(spatial, truth, obj) for x in (out, out_plain))
    r_static, r_static_plain = (_relmse(x, truth, static) / _relmse(spatial, truth, static) for x in (out, out_plain))
    print("%d object pixels: relMSE temporal / spatial with motion %.3f, without %.3f; mean history with motion %.2f, without %.2f" % (
        obj.sum(), r_obj, r_obj_plain, n[obj].mean(), n_plain[obj].mean()))
    print("%d static pixels: relMSE temporal / spatial with motion %.3f, without %.3f" % (static.sum(), r_static, r_static_plain))
    assert r_obj < 1.0
    assert r_static <= 1.05 * r_static_plain
