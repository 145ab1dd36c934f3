"""Motion-aware temporal denoising without a GPU (include/pt_motion.h): pt_motion_table against numpy float64 and the
contract's classification, the restatement tests/temporal_motion_ref.py against tests/temporal_ref.py bit for bit where nothing moves, the
symbols and their declarations, and every refusal that needs no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from cpupathtrace_amd import binding, build, scenes
from tests import denoise_ref, mesh_cases, motion_ref, temporal_motion_ref, temporal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_OK, PT_ERR_INVALID, PT_ERR_NO_DEVICE = 0, 1, 2
F = np.float32
PROJECTIVE = mesh_cases.TRANSFORMS["projective"]
SMALL_IN_BOX = np.array([[0.015, 0, 0, 0.1], [0, 0.02, 0, -0.1], [0, 0, 0.015, 0.2], [0, 0, 0, 1]], F)  # tests/test_gpu_pose.py's


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

def _rotation(axis, degrees):
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(4)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def _affine(linear, translation):
    m = np.eye(4)
    m[:3, :3] = linear
    m[:3, 3] = translation
    return m.astype(F)


def matrix_set():
    """fp32 matrices: rotations about the three axes x uniform scales 0.4 .. 2 x translations within +-2, a non-uniform scale, a mirror
    (negative determinant), and the projective and the small-in-box matrix of the pose tests."""
    rng = np.random.default_rng(41)
    out = []
    for axis in range(3):
        for scale in (0.4, 0.75, 1.0, 1.3, 2.0):
            out.append(_affine(_rotation(axis, rng.uniform(-170, 170))[:3, :3] * scale, rng.uniform(-2, 2, 3)))
    out.append(_affine(np.diag([1.0, 0.5, 2.0]), (0.3, -1.0, 0.7)))
    out.append(_affine(np.diag([-1.0, 1.0, 1.0]) @ _rotation(1, 33.0)[:3, :3], (1.5, 0.2, -0.4)))
    out.append(np.array(SMALL_IN_BOX, F))
    out.append(np.array(PROJECTIVE, F))
    return out


def _families():
    """(family, current, previous, expected kind) over all pairs of the set and the special previous matrices."""
    ms = matrix_set()
    nan, inf = np.array(ms[0]), np.array(ms[1])
    nan[1, 2] = np.nan
    inf[0, 3] = np.inf
    singular = _affine(np.array([[1, 2, 3], [2, 4, 6], [0, 1, 0]], np.float64), (0, 0, 0))  # rank 2: the determinant is exactly 0
    cases = []
    for i, c in enumerate(ms):
        for j, p in enumerate(ms):
            projective = (c[3] != np.array([0, 0, 0, 1], F)).any() or (p[3] != np.array([0, 0, 0, 1], F)).any()
            if i == j:
                cases.append(("static", c, p.copy(), motion_ref.STATIC))
            elif projective:
                cases.append(("projective", c, p, motion_ref.NONE))
            else:
                cases.append(("moved", c, p, motion_ref.MOVED))
        if (c[3] == np.array([0, 0, 0, 1], F)).all():
            cases.append(("non-finite", c, nan, motion_ref.NONE))
            cases.append(("non-finite", c, inf, motion_ref.NONE))
            cases.append(("non-finite", c, np.full((4, 4), np.nan, F), motion_ref.NONE))
            cases.append(("singular", c, singular, motion_ref.NONE))
            cases.append(("singular", singular, c, motion_ref.NONE))
    return cases


def test_motion_table_matches_float64(lib):
    cases = _families()
    assert {f for f, _, _, _ in cases} == {"static", "moved", "projective", "non-finite", "singular"}
    cur = np.stack([c for _, c, _, _ in cases])
    prev = np.stack([p for _, _, p, _ in cases])
    kind, back, normal = binding.motion_table(cur, prev)
    worst = 0.0
    for k, (family, c, p, want) in enumerate(cases):
        assert motion_ref.classify(c, p) == want, family  # (the restated classification agrees with the family's construction)
        assert kind[k] == want, (family, k, kind[k], c, p)
        if want == motion_ref.MOVED:
            b64, n64 = motion_ref.table64(c, p)
            for got, ref in ((back[k], b64), (normal[k], n64)):
                bound = 2.0 ** -23 * np.abs(ref).max()
                err = np.abs(got.astype(np.float64) - ref.astype(F).astype(np.float64)).max()
                worst = max(worst, err / bound)
                assert err <= bound, (family, k, err, bound)
        elif want == motion_ref.STATIC:
            assert (back[k] == np.eye(4, dtype=F)[:3]).all() and (normal[k] == np.eye(3, dtype=F)).all()
        else:
            assert (back[k] == 0).all() and (normal[k] == 0).all()
    print("%d cases, %d moved; largest error %.3f of the bound" % (len(cases), int((kind == 1).sum()), worst))


def test_moved_determinants_are_well_conditioned():
    """What the bound of the test above rests on: |det| >= 0.06 for every affine matrix of the set but the small-in-box one, whose
    determinant (4.5e-6) is small by its scale alone (its condition number is 4/3)."""
    for m in matrix_set():
        if (m[3] != np.array([0, 0, 0, 1], F)).any():
            continue
        a = m[:3, :3].astype(np.float64)
        if np.array_equal(m, SMALL_IN_BOX):
            assert np.linalg.cond(a) < 1.4
        else:
            assert abs(np.linalg.det(a)) >= 0.06 and np.linalg.cond(a) <= 4.0 + 1e-9


def test_motion_table_takes_points_and_normals_back():
    """The meaning of the table: back takes C x to P x, and normal takes the normal of a plane under C to that plane's normal under P."""
    ms = [m for m in matrix_set() if (m[3] == np.array([0, 0, 0, 1], F)).all()]
    rng = np.random.default_rng(5)
    cur, prev = np.stack(ms[:-1]), np.stack(ms[1:])
    kind, back, normal = binding.motion_table(cur, prev)
    assert (kind == 1).all()
    x = rng.uniform(-1, 1, (16, 3))
    u, v = rng.normal(size=(16, 3)), rng.normal(size=(16, 3))
    for c, p, b, n in zip(cur.astype(np.float64), prev.astype(np.float64), back.astype(np.float64), normal.astype(np.float64)):
        here, there = x @ c[:3, :3].T + c[:3, 3], x @ p[:3, :3].T + p[:3, 3]
        np.testing.assert_allclose(here @ b[:, :3].T + b[:, 3], there, rtol=0, atol=2e-5 * max(1.0, np.abs(there).max()))
        n_here = np.cross(u @ c[:3, :3].T, v @ c[:3, :3].T)
        n_there = np.cross(u @ p[:3, :3].T, v @ p[:3, :3].T)
        got = n_here @ n.T
        cosine = np.sum(got * n_there, axis=1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(n_there, axis=1))
        # (the cofactor matrix: a mirror between the two poses flips the cross product's hand, not the plane)
        np.testing.assert_allclose(np.abs(cosine), 1.0, rtol=0, atol=1e-5)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------

def _orbit(cam, degrees):
    o, la = np.asarray(cam["origin"], np.float64), np.asarray(cam["look_at"], np.float64)
    a = math.radians(degrees)
    d = o - la
    rot = np.array([d[0] * math.cos(a) + d[2] * math.sin(a), d[1], -d[0] * math.sin(a) + d[2] * math.cos(a)])
    return dict(cam, origin=tuple(float(v) for v in la + rot))


def _pan(cam, dx):
    o, la = cam["origin"], cam["look_at"]
    return dict(cam, origin=(o[0] + dx, o[1], o[2]), look_at=(la[0] + dx, la[1], la[2]))


@pytest.mark.parametrize("kind", ["static", "pan", "orbit"])
def test_restatement_without_motion_is_temporal_ref(oracle_lib, kind):
    """temporal_motion_ref.push with motion None and with the all-static motion built from the features equals temporal_ref.push bit for
    bit, outputs and history lengths, on noisy synthetic frames over oracle features of the Cornell box."""
    w, h = 24, 20
    sc, cam = scenes.cornell_scene(w, h)
    cams = {"static": [cam] * 4, "pan": [_pan(cam, 0.03 * k) for k in range(4)], "orbit": [_orbit(cam, 1.5 * k) for k in range(4)]}[kind]
    feats = {}
    rng = np.random.default_rng(13)
    for p in (temporal_ref.params(), temporal_ref.params(spatial={"iterations": 2, "sigma_luminance": 8.0}, max_history=3, moments_min_history=2, normal_min=0.8)):
        states = [temporal_ref.TemporalState() for _ in range(3)]
        longest = 0
        for v, c in enumerate(cams):
            if v not in feats:
                feats[v] = denoise_ref.host_features(oracle_lib, sc, c, w, h)
            feat = feats[v]
            rgba = np.ones((h, w, 4), F)
            rgba[..., :3] = rng.uniform(0.5, 1.5, (h, w, 3)).astype(F) * np.maximum(feat[..., 0, :3], 0.01)
            want, wn = temporal_ref.push(states[0], rgba, feat, c, p)
            for state, motion in ((states[1], None), (states[2], temporal_motion_ref.static_motion(feat))):
                got, n = temporal_motion_ref.push(state, rgba, feat, motion, c, p)
                assert np.array_equal(n, wn)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            longest = max(longest, int(wn.max()))
        assert longest >= 3  # (histories did grow: the equality is not one of first pushes)


def test_restatement_follows_a_moved_point():
    """One plane pixel, hand-made: under the same camera a pixel whose motion says "was one pixel to the left" takes its history from
    there; a pixel with no previous position starts anew; what is stored for the next push is the current surface."""
    w, h = 8, 6
    cam = scenes.camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -float(w) / h)
    ys, xs = np.mgrid[0:h, 0:w]
    # a wall at z = 0 seen from z = -3: what pixel (x, y) sees, checked with the projection itself (the sign of x is the aspect ratio's)
    step = 3.0 * abs(cam["height"] * cam["aspect_ratio"]) / cam["focal_length"] / w
    X = np.zeros((h, w, 3), F)
    X[..., 0] = ((xs + 0.5) / w - 0.5) * step * w
    X[..., 1] = -((ys + 0.5) / h - 0.5) * (3.0 * cam["height"] / cam["focal_length"])
    px, py, found = temporal_ref.project(X, cam, w, h)
    sign = 1.0 if abs(px[0, 1] - 1.0) < 1e-3 else -1.0
    X[..., 0] *= sign
    px, py, found = temporal_ref.project(X, cam, w, h)
    assert found.all() and np.abs(px - xs).max() < 1e-3 and np.abs(py - ys).max() < 1e-3
    feat = np.zeros((h, w, 3, 4), F)
    feat[..., 0, :] = (0.5, 0.5, 0.5, 1.0)
    feat[..., 1, :] = (0, 0, -1, 3.0)
    feat[..., 2, :3] = X
    rng = np.random.default_rng(2)
    frames = [np.concatenate([rng.uniform(0.2, 0.8, (h, w, 3)), np.ones((h, w, 1))], axis=-1).astype(F) for _ in range(2)]
    p = temporal_ref.params(spatial={"iterations": 0})
    state = temporal_ref.TemporalState()
    temporal_motion_ref.push(state, frames[0], feat, temporal_motion_ref.static_motion(feat), cam, p)
    motion = temporal_motion_ref.static_motion(feat)
    motion[2, 4, 0, :3] = X[2, 3]  # pixel (4, 2) was where pixel (3, 2) is
    motion[2, 4, 0, 3] = 1.0
    motion[3, 5, 1, 3] = 0.25      # one ray of pixel (5, 3) had no previous position
    stored = state.prev
    out, n = temporal_motion_ref.push(state, frames[1], feat, motion, cam, p)
    assert n[3, 5] == 1 and n[2, 4] == 2 and (np.delete(n.ravel(), [3 * w + 5]) == 2).all()
    c1 = denoise_ref.prepare(frames[1], feat)[0]
    a = F(0.5)
    np.testing.assert_allclose(state.prev["col"][2, 4], (F(1) - a) * stored["col"][2, 3] + a * c1[2, 4], rtol=2e-3)  # (px = 3 to 1e-3 px)
    np.testing.assert_allclose(state.prev["col"][2, 2], (F(1) - a) * stored["col"][2, 2] + a * c1[2, 2], rtol=1e-6)
    assert np.array_equal(state.prev["pos"], X) and np.array_equal(state.prev["col"][3, 5], c1[3, 5])


# ---- the ABI without a device ----------------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_declared():
    build.build()
    lib = C.CDLL(binding.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pt_motion.h")).read()
    declared = set(re.findall(r"^int (pt_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(binding.MOTION_EXPORTS) == {"pt_motion_table", "pt_render_features_motion", "pt_render_features_motion_device",
                                                       "pt_temporal_denoise_motion", "pt_temporal_denoise_motion_device"}
    for other in (binding.EXPORTS, binding.MESH_EXPORTS, binding.POSE_EXPORTS, binding.FEATURES_EXPORTS):
        assert not declared & set(other)
    for name in declared:
        assert hasattr(lib, name), name
    top = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert top.index('#include "pt_pose.h"') < top.index('#include "pt_motion.h"')
    assert (binding.MOTION_STATIC, binding.MOTION_MOVED, binding.MOTION_NONE) == (0, 1, 2)
    assert re.search(r"PT_MOTION_STATIC = 0, PT_MOTION_MOVED = 1, PT_MOTION_NONE = 2", header)
    for word in ("view batches", "followed features"):  # what is left out is named
        assert word in header


def test_refusals_come_before_any_device(lib):
    P = binding._ptr
    m = np.eye(4, dtype=F).reshape(1, 16)
    kind, back, normal = np.zeros(1, np.uint8), np.zeros((1, 12), F), np.zeros((1, 9), F)
    n1 = C.c_uint32(1)
    assert lib.pt_motion_table(None, P(m), n1, P(kind), P(back), P(normal)) == PT_ERR_INVALID
    assert lib.pt_motion_table(P(m), None, n1, P(kind), P(back), P(normal)) == PT_ERR_INVALID
    assert lib.pt_motion_table(P(m), P(m), n1, None, P(back), P(normal)) == PT_ERR_INVALID
    assert lib.pt_motion_table(P(m), P(m), n1, P(kind), None, P(normal)) == PT_ERR_INVALID
    assert lib.pt_motion_table(P(m), P(m), n1, P(kind), P(back), None) == PT_ERR_INVALID
    assert lib.pt_motion_table(None, None, C.c_uint32(0), None, None, None) == PT_OK
    assert lib.pt_motion_table(P(m), P(m), n1, P(kind), P(back), P(normal)) == PT_OK  # (no device is needed)
    # the feature pass: a null scene, before its other arguments are looked at
    cam, opt = binding._camera(scenes.box_scene()[1]), binding._options(scenes.options(8, 6, 1, 1))
    feat, mot = np.zeros((6, 8, 3, 4), F), np.zeros((6, 8, 2, 4), F)
    assert lib.pt_render_features_motion(None, C.byref(cam), C.byref(opt), None, P(feat), P(mot)) == PT_ERR_INVALID
    assert lib.pt_render_features_motion_device(None, C.byref(cam), C.byref(opt), None, P(feat), P(mot), None) == PT_ERR_INVALID
    # the push: null arguments and a degenerate camera (the handle is never dereferenced)
    dummy = C.create_string_buffer(256)
    img, out, hist = np.zeros((6, 8, 4), F), np.zeros((6, 8, 4), F), np.zeros((6, 8), np.int32)

    def call(t=C.addressof(dummy), rgba=img, features=feat, motion=mot, camera=cam, o=out, on_device=False):
        args = (C.c_void_p(t) if t else None, P(rgba), P(features), P(motion), C.byref(camera) if camera is not None else None, P(o), P(hist))
        return lib.pt_temporal_denoise_motion_device(*args, None) if on_device else lib.pt_temporal_denoise_motion(*args)

    for on_device in (False, True):
        bad = [call(t=None, on_device=on_device), call(rgba=None, on_device=on_device), call(features=None, on_device=on_device),
               call(camera=None, on_device=on_device), call(o=None, on_device=on_device),
               call(camera=binding._camera(dict(scenes.box_scene()[1], up=(0, 0, 0))), on_device=on_device)]
        assert bad == [PT_ERR_INVALID] * len(bad), bad
    assert (feat == 0).all() and (mot == 0).all() and (out == 0).all()


def test_without_a_device_there_is_no_scene_to_ask():
    """With every argument in order the answer depends on the machine: a scene, and with it the feature pass, needs a device."""
    if binding.device_count() > 0:
        return  # (tests/test_gpu_motion.py)
    with pytest.raises(binding.PtError) as e:
        binding.Scene(scenes.box_scene()[0])
    assert e.value.code == PT_ERR_NO_DEVICE
    with pytest.raises(binding.PtError) as e:
        binding.TemporalDenoiser(8, 6)
    assert e.value.code == PT_ERR_NO_DEVICE


def test_binding_checks_shapes():
    with pytest.raises(ValueError):
        binding.motion_table(np.zeros((2, 4, 4), F), np.zeros((3, 4, 4), F))
    import inspect
    assert list(inspect.signature(binding.TemporalDenoiser.denoise).parameters) == ["self", "image", "features", "camera", "motion"]
    assert inspect.signature(binding.TemporalDenoiser.denoise).parameters["motion"].default is None
    assert inspect.signature(binding.TemporalDenoiser.denoise_device).parameters["motion"].default is None
    assert list(inspect.signature(binding.Scene.render_features_motion).parameters) == ["self", "camera", "options", "previous"]
    assert list(inspect.signature(binding.Scene.denoise_sequence).parameters) == ["self", "frames", "cameras", "options", "params", "poses"]


def test_cpp_program_compiles_and_links(tmp_path):
    from cpupathtrace_amd import build_host
    exe = str(tmp_path / "motion_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "motion_test.cpp")], exe, extra_flags=["-O1"])
    assert os.path.exists(exe)
    header = open(os.path.join(ROOT, "include", "PathTrace", "temporal_denoise.h")).read()
    fields = re.search(r"struct TemporalDenoiseParams \{(.*?)\n\};", header, re.S).group(1)
    assert re.sub(r"//.*", "", fields).split(";")[-2].strip() == "bool follow_motion = false"  # the last field, off by default
