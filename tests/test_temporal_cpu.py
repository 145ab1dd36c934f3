"""CPU checks of temporal denoising (pt_temporal_*, binding.TemporalDenoiser, include/PathTrace/temporal_denoise.h): the exports and defaults,
the library's refusal of bad arguments before anything touches a device, the C++ header compiles and links, and properties of the numpy
restatement (tests/temporal_ref.py) the GPU is checked against, on features the CPU oracle traces."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build, build_host, scenes
from tests import denoise_ref, temporal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_OK, PT_ERR_INVALID, PT_ERR_NO_DEVICE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def test_symbols_are_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(binding.TEMPORAL_EXPORTS) <= names
    assert set(binding.TEMPORAL_EXPORTS) <= set(binding.EXPORTS)
    header = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    for name in binding.TEMPORAL_EXPORTS:
        assert name + "(" in header


def test_default_parameters(lib):
    p = binding.TemporalParams()
    assert lib.pt_temporal_params_default(C.byref(p)) == PT_OK
    assert p.as_dict() == temporal_ref.DEFAULTS
    assert binding.temporal_params_default() == temporal_ref.DEFAULTS
    assert temporal_ref.DEFAULTS["spatial"] == binding.denoise_params_default()
    assert (p.alpha_color, p.alpha_moments, p.max_history, p.moments_min_history) == (np.float32(0.2), np.float32(0.2), 32, 4)
    assert lib.pt_temporal_params_default(None) == PT_ERR_INVALID


def _params(**kw):
    p = binding._temporal_params({})
    for k, v in kw.items():
        if k in ("iterations", "sigma_luminance", "sigma_normal", "sigma_depth"):
            setattr(p.spatial, k, v)
        else:
            setattr(p, k, v)
    return p


def test_create_refuses_bad_arguments(lib):
    def call(width=8, height=6, params=None, out=True, device=0):
        h = C.c_void_p()
        rc = lib.pt_temporal_create(C.c_int(device), C.c_int32(width), C.c_int32(height), C.byref(params) if params is not None else None,
                                    C.byref(h) if out else None)
        if rc == PT_OK:
            lib.pt_temporal_destroy(h)
        return rc

    bad = [call(out=False), call(width=0), call(height=0), call(width=-3), call(width=16384, height=16385),
           call(params=_params(alpha_color=0.0)), call(params=_params(alpha_color=1.5)), call(params=_params(alpha_moments=-0.1)),
           call(params=_params(alpha_moments=math.nan)), call(params=_params(max_history=0)), call(params=_params(moments_min_history=0)),
           call(params=_params(iterations=11)), call(params=_params(sigma_luminance=-1.0)), call(params=_params(sigma_normal=math.inf)),
           call(params=_params(sigma_luminance_temporal=-2.0)), call(params=_params(sigma_luminance_temporal=math.nan)),
           call(params=_params(position_tolerance=-1.0)), call(params=_params(position_tolerance=math.inf)),
           call(params=_params(normal_min=math.nan))]
    assert bad == [PT_ERR_INVALID] * len(bad), bad
    want = PT_OK if binding.device_count() > 0 else PT_ERR_NO_DEVICE
    assert call() == want
    assert call(params=_params(alpha_color=1.0, max_history=1, moments_min_history=1, position_tolerance=0.0, normal_min=-2.0)) == want


def _cam(**kw):
    return binding._camera(dict(scenes.box_scene()[1], **kw))


BAD_CAMERAS = {"look_at = origin": dict(look_at=(0, 0, -3)), "zero up": dict(up=(0, 0, 0)), "up along the view": dict(up=(0, 0, 1)),
               "zero focal length": dict(focal_length=0.0), "zero height": dict(height=0.0), "zero aspect ratio": dict(aspect_ratio=0.0),
               "nan origin": dict(origin=(math.nan, 0, -3)), "infinite focal length": dict(focal_length=math.inf)}


def test_push_refuses_bad_arguments(lib):
    dummy = C.create_string_buffer(256)  # (never dereferenced: every case below fails before the handle is used)
    img = np.zeros((6, 8, 4), np.float32)
    feat = np.zeros((6, 8, 3, 4), np.float32)
    out = np.zeros_like(img)
    hist = np.zeros((6, 8), np.int32)
    P = binding._ptr

    def call(t=C.addressof(dummy), rgba=img, features=feat, camera=_cam(), o=out, on_device=False):
        args = (C.c_void_p(t) if t else None, P(rgba), P(features), C.byref(camera) if camera is not None else None, P(o), P(hist))
        return lib.pt_temporal_denoise_device(*args, None) if on_device else lib.pt_temporal_denoise(*args)

    for on_device in (False, True):
        bad = [call(t=None, on_device=on_device), call(rgba=None, on_device=on_device), call(features=None, on_device=on_device),
               call(camera=None, on_device=on_device), call(o=None, on_device=on_device)]
        bad += [call(camera=_cam(**kw), on_device=on_device) for kw in BAD_CAMERAS.values()]
        assert bad == [PT_ERR_INVALID] * len(bad), bad
    assert lib.pt_temporal_reset(None) == PT_ERR_INVALID
    assert lib.pt_temporal_destroy(None) == PT_ERR_INVALID
    with pytest.raises(ValueError):
        binding._temporal_params({"alpha": 0.5})
    with pytest.raises(ValueError):
        binding._temporal_params({"spatial": {"iterationz": 3}})


def test_restatement_refuses_degenerate_cameras():
    for what, kw in BAD_CAMERAS.items():
        if "nan" in what or "infinite" in what:
            continue
        assert temporal_ref.camera_rows(dict(scenes.box_scene()[1], **kw)) is None, what


def test_cpp_program_compiles_and_links(tmp_path):
    exe = str(tmp_path / "temporal_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "temporal_test.cpp")], exe, extra_flags=["-O1"])
    assert os.path.exists(exe)
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    assert "TemporalDenoiser::push(Image<Color<float> > const&, Camera const&)" in out
    assert "denoiseSequence(" in out


# ---- properties of the restatement, on oracle features -----------------------------------------------------------------------------

def _flat_interior(feat):
    """Fully covered pixels whose 3x3 neighbourhood is fully covered with one normal: the 4 feature rays hit one plane."""
    cov, n = feat[..., 0, 3], feat[..., 1, :3]
    h, w = cov.shape
    ok = cov == 1
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            cs, _ = denoise_ref._shift(cov, dx, dy)
            ns, m = denoise_ref._shift(n, dx, dy)
            ok &= m & (cs == 1) & (np.abs(ns - n).max(axis=-1) < 1e-6)
    return ok


def _cornell_features(oracle_lib, cam, w, h):
    sc, _ = scenes.cornell_scene(w, h)
    return denoise_ref.host_features(oracle_lib, sc, cam, w, h)


def _camera_of(kind, w, h):
    _, cam = scenes.cornell_scene(w, h)  # thin lens, aspect ratio -w/h as the demo's
    if kind == "pinhole":
        cam = dict(cam, aperture_kind=scenes.APERTURE_NONE, aperture_width=0.0, aperture_height=0.0, focal_plane_dist=0.0)
    elif kind == "aspect+1":
        cam = dict(cam, aspect_ratio=-cam["aspect_ratio"])
    elif kind == "skewed_up":  # up not perpendicular to the view
        cam = dict(cam, up=(0.3, 1.0, -0.4), origin=(0.2, 0.1, -2.9))
    return cam


@pytest.mark.parametrize("kind", ["pinhole", "thin_lens", "aspect+1", "skewed_up"])
def test_projection_of_own_positions(oracle_lib, kind):
    """Points along each feature ray project onto that ray's sub-pixel position, and a pixel's mean hit position onto its centre where the
    surface faces the camera (on an oblique plane the mean of 4 hits is off the centre by the perspective: up to 0.02 px at 40 x 32)."""
    w, h = 40, 32
    cam = _camera_of(kind, w, h)
    assert temporal_ref.camera_rows(cam) is not None
    ys, xs = np.mgrid[0:h, 0:w]
    rays = denoise_ref.feature_rays(oracle_lib, cam, w, h)
    for (dx, dy), r in zip(denoise_ref.SUBPIXEL, rays):
        for s in (0.5, 3.0):
            pts = (r[:, :3] + r[:, 3:] * np.float32(s)).astype(np.float32).reshape(h, w, 3)
            px, py, found = temporal_ref.project(pts, cam, w, h)
            assert found.all()
            err = np.maximum(np.abs(px - (xs + dx)), np.abs(py - (ys + dy)))
            assert err.max() <= 1e-3, (dx, dy, s, err.max())
    feat = _cornell_features(oracle_lib, cam, w, h)
    X, n, _ = temporal_ref.surface(feat)
    px, py, found = temporal_ref.project(X, cam, w, h)
    view = temporal_ref.camera_basis(cam)[1]
    facing = _flat_interior(feat) & (np.abs(n @ (view / np.linalg.norm(view))) > 0.99)
    assert facing.sum() >= 20
    err = np.maximum(np.abs(px - xs), np.abs(py - ys))[facing]
    print("%s: %d pixels facing the camera, largest distance %.3g px" % (kind, facing.sum(), err.max()))
    assert found[facing].all() and err.max() <= 1e-3


def _noisy(rng, feat, level=0.5):
    h, w = feat.shape[:2]
    rgba = np.ones((h, w, 4), np.float32)
    rgba[..., :3] = rng.uniform(1.0 - level, 1.0 + level, (h, w, 3)).astype(np.float32) * np.maximum(feat[..., 0, :3], 0.01)
    return rgba


def test_static_camera_blends_in_closed_form(oracle_lib):
    w, h = 24, 20
    _, cam = scenes.cornell_scene(w, h)
    feat = _cornell_features(oracle_lib, cam, w, h)
    rng = np.random.default_rng(7)
    p = temporal_ref.params(spatial={"iterations": 0}, max_history=3)
    state = temporal_ref.TemporalState()
    c_hist = None
    covered = feat[..., 0, 3] > 0
    for k in range(1, 6):
        rgba = _noisy(rng, feat)
        c, _, _, _, factor = denoise_ref.prepare(rgba, feat)
        out, n = temporal_ref.push(state, rgba, feat, cam, p)
        assert (n[covered] == min(k, 3)).all() and (n[~covered] == 0).all()
        if k == 1:
            want = c
        else:
            nn = np.float32(min(k, 3))
            a = max(np.float32(1.0) / nn, np.float32(0.2))
            want = ((np.float32(1.0) - a) * c_hist + a * c).astype(np.float32)
        want = np.where(covered[..., None], want, c)
        np.testing.assert_array_equal(state.prev["col"], want)
        c_hist = want
        np.testing.assert_array_equal(out[..., :3], want * factor)


def test_first_push_is_the_spatial_filter(oracle_lib):
    w, h = 24, 20
    _, cam = scenes.cornell_scene(w, h)
    feat = _cornell_features(oracle_lib, cam, w, h)
    rng = np.random.default_rng(3)
    rgba = _noisy(rng, feat)
    for p in (temporal_ref.params(), temporal_ref.params(spatial={"iterations": 2, "sigma_luminance": 8.0}, moments_min_history=1)):
        state = temporal_ref.TemporalState()
        out, n = temporal_ref.push(state, rgba, feat, cam, p)
        np.testing.assert_array_equal(out, denoise_ref.denoise(rgba, feat, **p["spatial"]))
        state.reset()
        out2, _ = temporal_ref.push(state, rgba, feat, cam, p)
        np.testing.assert_array_equal(out2, out)
        assert set(np.unique(n)) <= {0, 1}


def test_constant_irradiance_is_kept(oracle_lib):
    w, h = 24, 20
    _, cam = scenes.cornell_scene(w, h)
    feat = _cornell_features(oracle_lib, cam, w, h)
    rgba = np.ones((h, w, 4), np.float32)
    rgba[..., :3] = np.float32(0.7) * np.maximum(feat[..., 0, :3], 0.01)
    rgba[..., :3] = np.where(feat[..., 0, 3:] > 0, rgba[..., :3], np.float32(0.0))
    state = temporal_ref.TemporalState()
    cams = [cam, dict(cam, origin=(0.02, 0.0, -3.0)), dict(cam, origin=(0.04, 0.01, -3.0))]
    for k, cm in enumerate(cams * 2):
        f = _cornell_features(oracle_lib, cm, w, h)
        rgba = np.ones((h, w, 4), np.float32)
        rgba[..., :3] = np.where(f[..., 0, 3:] > 0, np.float32(0.7) * np.maximum(f[..., 0, :3], 0.01), np.float32(0.0))
        out, n = temporal_ref.push(state, rgba, f, cm)
        np.testing.assert_allclose(out, rgba, rtol=1e-5, atol=1e-7)
        if k > 0:
            assert (n > 1).sum() > 0.5 * (n > 0).sum()
