"""Followed features (include/pt_features.h) without a GPU: the exports and their declarations, the defaults, every refusal
before anything is uploaded, the C++ program, the pin of the restated glass branches (tests/features_follow_ref.py) to the oracle, and the
properties of the restatement on the scene set."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build, build_host, scenes
from tests import denoise_ref
from tests import features_follow_ref as ffr
from tests import unit_cases as uc
from tests.util import assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1

DECLARATIONS = {
    "pt_feature_params_default": "int pt_feature_params_default(pt_feature_params *out);",
    "pt_render_features_followed": "int pt_render_features_followed(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, "
                                   "const pt_feature_params *params, float *out_features);",
    "pt_render_features_followed_device": "int pt_render_features_followed_device(pt_scene *scene, const pt_camera_params *camera, const pt_options *options, "
                                          "const pt_feature_params *params, float *d_out_features, void *stream);",
    "pt_render_features_followed_views": "int pt_render_features_followed_views(pt_scene *scene, const pt_camera_params *cameras, int32_t n_views, "
                                         "const pt_options *options, const pt_feature_params *params, float *out_features);",
    "pt_render_features_followed_views_device": "int pt_render_features_followed_views_device(pt_scene *scene, const pt_camera_params *cameras, int32_t n_views, "
                                                "const pt_options *options, const pt_feature_params *params, float *d_out_features, void *stream);",
    "pt_frame_set_feature_params": "int pt_frame_set_feature_params(pt_frame *frame, const pt_feature_params *params /* NULL = first-hit features */);",
}


@pytest.fixture(scope="module")
def lib():
    build.build()
    return C.CDLL(binding.LIB_PATH)


def test_symbols_are_exported_and_declared(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(binding.FEATURES_EXPORTS) == set(DECLARATIONS)
    assert set(binding.FEATURES_EXPORTS) <= names
    header = " ".join(open(os.path.join(ROOT, "include", "pt_features.h")).read().split())
    for name, decl in DECLARATIONS.items():
        assert " ".join(decl.split()) in header, name
    assert '#include "pt_features.h"' in open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert not set(binding.FEATURES_EXPORTS) & set(binding.EXPORTS)  # (EXPORTS is what pt_hip.h itself declares)


def test_defaults_and_struct(lib):
    p = binding.FeatureParams()
    assert C.sizeof(p) == 8
    assert lib.pt_feature_params_default(C.byref(p)) == 0
    assert (p.max_bounces, p.flags) == (8, 0)
    assert binding.feature_params_default() == {"max_bounces": 8, "flags": 0}
    assert lib.pt_feature_params_default(None) == PT_ERR_INVALID
    with pytest.raises(ValueError):
        binding._feature_params({"bounces": 3})
    assert binding._feature_params({"max_bounces": 3}).max_bounces == 3 and binding._feature_params({}).max_bounces == 8
    header = open(os.path.join(ROOT, "include", "pt_features.h")).read()
    assert "int32_t max_bounces; /* 0..32, default 8 */" in header and "int32_t flags;" in header


def test_render_entries_refuse_bad_arguments(lib):
    dummy = C.create_string_buffer(64)  # (never dereferenced: every check below fails before a scene is used)
    cam = binding._camera(scenes.box_scene()[1])
    out = np.zeros((3, 6, 8, 3, 4), np.float32)
    good = binding.FeatureParams(8, 0)

    def call(form, scene=C.addressof(dummy), camera=cam, opt=scenes.options(8, 6, 1, 1), params=good, o=out, n_views=1):
        op = binding._options(opt)
        head = (C.c_void_p(scene) if scene else None, C.byref(camera) if camera is not None else None)
        tail = (C.byref(op), C.byref(params) if params is not None else None, binding._ptr(o))
        if form == "host":
            return lib.pt_render_features_followed(*head, *tail)
        if form == "device":
            return lib.pt_render_features_followed_device(*head, *tail, None)
        if form == "views":
            return lib.pt_render_features_followed_views(*head, C.c_int32(n_views), *tail)
        return lib.pt_render_features_followed_views_device(*head, C.c_int32(n_views), *tail, None)

    for form in ("host", "device", "views", "views_device"):
        bad = [call(form, scene=None), call(form, camera=None), call(form, o=None),
               call(form, opt=scenes.options(0, 6, 1, 1)), call(form, opt=scenes.options(8, -1, 1, 1)), call(form, opt=scenes.options(16384, 16385, 1, 1)),
               call(form, params=binding.FeatureParams(-1, 0)), call(form, params=binding.FeatureParams(33, 0)), call(form, params=binding.FeatureParams(8, 1)),
               call(form, opt=scenes.options(8, 6, 1, 1, epsilon=-1e-3)), call(form, opt=scenes.options(8, 6, 1, 1, epsilon=float("nan"))),
               call(form, opt=scenes.options(8, 6, 1, 1, epsilon=float("inf")))]
        assert bad == [PT_ERR_INVALID] * len(bad), (form, bad)
    for form in ("views", "views_device"):
        assert call(form, n_views=0) == PT_ERR_INVALID and call(form, n_views=-2) == PT_ERR_INVALID
    # NULL options with NULL parameters (the defaults) is still the null-argument refusal
    assert lib.pt_render_features_followed(C.c_void_p(C.addressof(dummy)), C.byref(cam), None, None, binding._ptr(out)) == PT_ERR_INVALID


def test_frame_entry_refuses_bad_arguments(lib):
    dummy = C.create_string_buffer(4096)  # (zeros: a frame whose epsilon is 0; nothing but its options is read before the refusal)
    good = binding.FeatureParams(8, 0)
    assert lib.pt_frame_set_feature_params(None, C.byref(good)) == PT_ERR_INVALID
    assert lib.pt_frame_set_feature_params(None, None) == PT_ERR_INVALID
    for p in (binding.FeatureParams(-1, 0), binding.FeatureParams(33, 0), binding.FeatureParams(0, 2)):
        assert lib.pt_frame_set_feature_params(C.c_void_p(C.addressof(dummy)), C.byref(p)) == PT_ERR_INVALID


def test_cpp_program_compiles_and_links(tmp_path):
    exe = str(tmp_path / "features_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "features_test.cpp")], exe, extra_flags=["-O1"])
    assert os.path.exists(exe)
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    assert "denoise(Image<Color<float> > const&, Scene const&, Camera const&, RenderOptions const&, DenoiseParams const&, FeatureParams const&)" in out
    assert "FrameRender::setFeatureParams(pt_feature_params const*)" in out
    assert "ViewBatchRender::setFeatureParams(pt_feature_params const*)" in out
    header = open(os.path.join(ROOT, "include", "PathTrace", "denoise.h")).read()
    assert "int max_bounces = 8;" in header


# ---- the restated glass branches against the oracle -----------------------------------------------------------------------------------

LEFT_OUT_CAP = 0.05
N_STATES = len(ffr.ENGINE_STATES)
glass_oracle_answers = ffr.glass_oracle_answers


@pytest.mark.parametrize("epsilon", uc.EPSILONS)
def test_glass_restatement_is_the_oracles(oracle_lib, epsilon):
    (rays, pos, nrm, ior), tir, outs, through = glass_oracle_answers(oracle_lib, epsilon)
    d = rays[:, 3:]
    assert tir.sum() > 100 and (~tir).sum() > 100
    # total internal reflection: every state reflects, and the restated reflection is that ray
    assert not through[:, tir].any()
    want = ffr.glass_reflect(d[tir], pos[tir], nrm[tir], ior[tir], epsilon)
    for k in range(N_STATES):
        assert_bits_equal(outs[k][:, :][tir], want, "reflection, state %d" % k)
    # everywhere else: a state that refracted
    rest = np.nonzero(~tir)[0]
    has = through[:, rest].any(axis=0)
    # the glass families are the last two parts of six (the critical angle +-{0, 1, 2} ulp, every ior, from inside and outside): the cap holds there
    n = len(rays)
    glass_parts = np.arange(n) >= uc._parts(n, 6)[4].start
    left_out = ((~tir) & glass_parts).sum() - has[glass_parts[rest]].sum()
    print("eps %g: %d cases reflect totally, %d do not; of the %d of the glass families %d (%.2f %%) have no refracting state among %d; of the other parts %d" % (
        epsilon, tir.sum(), len(rest), glass_parts.sum(), left_out, 100.0 * left_out / glass_parts.sum(), N_STATES, (~has[~glass_parts[rest]]).sum()))
    assert left_out <= LEFT_OUT_CAP * glass_parts.sum()
    # the other parts are pinned as well, where a state refracts.  Where none does there -- grazing incidence, |dot(d, n)| of 0 or a
    # denormal: the Fresnel reflectance is (-1)^2 = 1 although sin_theta_t < 1 -- the reference reflects with certainty: pd = 1 at every state
    never = rest[~has & ~glass_parts[rest]]
    pd = oracle_lib.bsdf_propagate(1, 0, rays[never], pos[never], nrm[never], epsilon, ior[never], np.full(len(never), ffr.ENGINE_STATES[4], np.uint64))[2]
    assert (pd == 1).all()
    sel = rest[has]
    first = through[:, sel].argmax(axis=0)
    got = ffr.glass_refract(d[sel], pos[sel], nrm[sel], ior[sel], epsilon)
    assert_bits_equal(got, outs[first, sel], "refraction")
    # and glass_follow picks between the two by sin_theta_t alone
    f_rays, f_refl = ffr.glass_follow(d, pos, nrm, ior, epsilon)
    assert (f_refl == tir).all()
    assert_bits_equal(f_rays[sel], got, "glass_follow, refraction")
    assert_bits_equal(f_rays[tir], want, "glass_follow, reflection")


# ---- properties of the restatement ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ffr.SCENE_SET))
def test_no_bounce_is_the_first_hit(oracle_lib, name):
    sc, cam, epsilon = ffr.scene(name)
    want = denoise_ref.host_features(oracle_lib, sc, cam, ffr.WIDTH, ffr.HEIGHT)
    assert_bits_equal(ffr.reference(oracle_lib, name, 0)[0], want, name)
    assert want[..., 0, 3].max() > 0
    if name not in ("mesh",):
        assert not np.array_equal(ffr.reference(oracle_lib, name, 8)[0], want)  # (the scenes show something specular)


def test_plane_mirror_gives_the_mirror_image(oracle_lib):
    """Through the plane mirror at x = 1 of the hall, a ray that ends on a diffuse surface after one bounce has the position of that hit
    point reflected across the mirror plane (x -> 2 - x) and the two segments' summed length."""
    sc, _, _ = ffr.scene("hall")
    # (a continued ray starts epsilon along its direction, so the unfolded position is short of the mirror image by epsilon per bounce:
    # 1e-5 here, below the tolerance; the scene set's 1e-3 would show as exactly that)
    epsilon = 1e-5
    cam = scenes.camera((-0.5, 0.1, -0.2), (1.0, 0.0, 0.7), (0, 1, 0), 1.0, 1.0, -1.2)  # (obliquely at the mirror: the image of the wall at z = 1)
    w, h = ffr.WIDTH, ffr.HEIGHT
    got = ffr.followed_features(oracle_lib, sc, cam, w, h, 1, epsilon).reshape(-1, 3, 4)
    handle = oracle_lib.scene_create(sc)
    mats = np.asarray(sc["materials"])
    pos_sum, t_sum, ok = np.zeros((w * h, 3)), np.zeros(w * h), np.ones(w * h, bool)
    for rays in denoise_ref.feature_rays(oracle_lib, cam, w, h):
        t0, o0 = handle.intersect(rays)
        p0 = rays[:, :3].astype(np.float64) + rays[:, 3:].astype(np.float64) * t0[:, None]
        _, m0 = handle.normal(o0, p0.astype(np.float32))
        on_mirror = (np.abs(p0[:, 0] - 1.0) < 1e-5) & (mats[np.minimum(m0, len(mats) - 1)]["bsdf"] == scenes.BSDF_MIRROR) & (m0 != scenes.NO_MATERIAL)
        d1 = rays[:, 3:].astype(np.float64) * np.array([-1.0, 1.0, 1.0])
        r1 = np.concatenate([p0 + d1 * epsilon, d1], axis=1).astype(np.float32)
        t1, o1 = handle.intersect(r1)
        p1 = r1[:, :3].astype(np.float64) + d1 * t1[:, None]
        _, m1 = handle.normal(o1, p1.astype(np.float32))
        diffuse = (m1 == scenes.NO_MATERIAL) | (mats[np.minimum(m1, len(mats) - 1)]["bsdf"] == scenes.BSDF_LAMBERTIAN)
        ok &= on_mirror & diffuse & (t1 >= 0)
        pos_sum += p1 * np.array([-1.0, 1.0, 1.0]) + np.array([2.0, 0.0, 0.0])
        t_sum += t0.astype(np.float64) + t1
    handle.close()
    assert ok.sum() >= 50, int(ok.sum())
    scene_size = 2.0
    assert np.abs(got[ok, 2, :3] - pos_sum[ok] / 4).max() <= 1e-4 * scene_size
    assert np.abs(got[ok, 1, 3] - t_sum[ok] / 4).max() <= 1e-4 * scene_size
    assert (got[ok, 0, 3] == 1).all()


def test_share_conditions(oracle_lib):
    shares = ffr.shares(oracle_lib)
    print({k: round(v, 4) for k, v in shares.items()})
    for key, least in ffr.SHARE_MIN.items():
        assert shares[key] >= least, (key, shares[key])


def test_bounded_and_deterministic(oracle_lib):
    """More bounces never change what fewer already ended: a pixel none of whose rays is capped at 2 is the same at 8 and at 32."""
    for name in ("hall", "glass", "one_way"):
        a, b, c = (ffr.reference(oracle_lib, name, mb)[0] for mb in (8, 32, 32))
        assert_bits_equal(b, c, name)
        sc, cam, epsilon = ffr.scene(name)
        again = ffr.followed_features(oracle_lib, sc, cam, ffr.WIDTH, ffr.HEIGHT, 8, epsilon)
        assert_bits_equal(again, a, name)
