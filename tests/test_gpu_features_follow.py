"""Followed features on the GPU (pt_render_features_followed*, pt_frame_set_feature_params; include/pt_features.h): the
device equals the restatement tests/features_follow_ref.py bit for bit on the scene set at every bounce limit, max_bounces 0 equals the
first-hit pass, the views and device-memory forms equal the single host form, a frame's denoised previews take the features they are told
to, bsdf_follow alone equals the oracle's state-selected answers, and the denoised frame gains what the CPU sweep measured."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cpupathtrace_amd import binding, scenes
from tests import denoise_ref
from tests import features_follow_ref as ffr
from tests import unit_cases as uc
from tests.util import assert_bits_equal, env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = ffr.WIDTH, ffr.HEIGHT
BOUNCES = [1, 2, 8, 32]


@pytest.fixture(scope="module")
def world():
    """One device scene per scene of the set, made on first use."""
    made = {}

    def get(name):
        if name not in made:
            sc, cam, epsilon = ffr.scene(name)
            made[name] = (binding.Scene(sc, device=0), cam, scenes.options(W, H, 1, 1, epsilon=epsilon))
        return made[name]

    yield get
    for gpu, _, _ in made.values():
        gpu.close()


@pytest.mark.parametrize("max_bounces", BOUNCES)
@pytest.mark.parametrize("name", list(ffr.SCENE_SET))
def test_device_equals_restatement(world, oracle_lib, name, max_bounces):
    gpu, cam, opt = world(name)
    got = gpu.render_features(cam, opt, followed={"max_bounces": max_bounces})
    assert_bits_equal(got, ffr.reference(oracle_lib, name, max_bounces)[0], "%s, %d bounces" % (name, max_bounces))


@pytest.mark.parametrize("name", list(ffr.SCENE_SET))
def test_no_bounce_is_the_first_hit_pass(world, name):
    gpu, cam, opt = world(name)
    assert_bits_equal(gpu.render_features(cam, opt, followed=binding.FeatureParams(0, 0)), gpu.render_features(cam, opt), name)


def test_records_in_lds_and_in_hbm(world):
    """The small scenes walk records staged in LDS, the mesh a device-built tree in HBM: both are among the scenes above."""
    assert world("hall")[0].info()["n_nodes"] < 64 and world("mesh")[0].info()["n_nodes"] >= 2 * 1024 - 1


def walk_calls(gpu, cam, opt, rays):
    """The calls that go through the walk kernels' dispatch beside the followed pass: first-hit features, single and views, and a ray batch."""
    return gpu.render_features(cam, opt), gpu.render_features_views(ffr.view_cameras(cam)[:2], opt), gpu.get_intersection(rays)


@pytest.mark.parametrize("knobs", [{"PT_LDS_SMALL": 0}, {"PT_STACK_WINDOW": 4}], ids=["records_in_hbm", "window_of_4"])
def test_other_instantiations_on_a_small_scene(oracle_lib, world, knobs):
    """A small scene with its records left in HBM, and staged in LDS with the 4-entry stack window: the same bits, from the followed pass
    and from the first-hit pass and intersect_batch (the frame's primary rays), which take the same route."""
    sc, cam, epsilon = ffr.scene("glass")
    opt = scenes.options(W, H, 1, 1, epsilon=epsilon)
    rays = denoise_ref.feature_rays(oracle_lib, cam, W, H).reshape(-1, 6)
    with env(**knobs):
        gpu = binding.Scene(sc, device=0)
        try:
            got = gpu.render_features(cam, opt, followed={"max_bounces": 8})
            views = gpu.render_features_views(ffr.view_cameras(cam)[:2], opt, followed={"max_bounces": 8})
            first, first_views, (t, obj) = walk_calls(gpu, cam, opt, rays)
        finally:
            gpu.close()
    assert_bits_equal(got, ffr.reference(oracle_lib, "glass", 8)[0], str(knobs))
    assert_bits_equal(views[0], got, "%s, view 0" % knobs)
    want_first, want_views, (want_t, want_obj) = walk_calls(world("glass")[0], cam, opt, rays)
    assert len(rays) == 4 * W * H and (want_obj >= 0).any()
    assert_bits_equal(first, want_first, "%s, first-hit features" % knobs)
    assert_bits_equal(first_views, want_views, "%s, first-hit features of two views" % knobs)
    assert_bits_equal(t, want_t, "%s, intersect_batch t" % knobs)
    assert_bits_equal(obj, want_obj, "%s, intersect_batch object" % knobs)


@pytest.mark.parametrize("name", list(ffr.SCENE_SET))
def test_views_equal_single_frames(world, name):
    gpu, cam, opt = world(name)
    cams = ffr.view_cameras(cam)
    got = gpu.render_features_views(cams, opt, followed={"max_bounces": 8})
    assert got.shape == (3, H, W, 3, 4)
    for v, c in enumerate(cams):
        assert_bits_equal(got[v], gpu.render_features(c, opt, followed={"max_bounces": 8}), "%s, view %d" % (name, v))
    assert not np.array_equal(got[0], got[1])
    assert_bits_equal(gpu.render_features_views(cams, opt, followed={"max_bounces": 0}), gpu.render_features_views(cams, opt), name + ", no bounce")


def test_default_parameters_are_eight_bounces(world):
    gpu, cam, opt = world("hall")
    assert_bits_equal(gpu.render_features(cam, opt, followed={}), gpu.render_features(cam, opt, followed={"max_bounces": 8}), "defaults")
    out = np.empty((H, W, 3, 4), np.float32)
    cp, op = binding._camera(cam), binding._options(opt)
    import ctypes as C
    binding._check(binding.load().pt_render_features_followed(gpu._h, C.byref(cp), C.byref(op), None, binding._ptr(out)))
    assert_bits_equal(out, gpu.render_features(cam, opt, followed={"max_bounces": 8}), "NULL parameters")


def test_share_conditions_on_the_device(world, oracle_lib):
    """The device's outputs at 8 bounces are the restatement's bit for bit, so what the restatement saw on its way to them is what the device
    did; what can be read off the outputs themselves is counted from them: a ray that escaped after a bounce is a quarter of coverage the
    first-hit pass has and the followed pass has not."""
    rays = lost = changed = 0
    for name in ffr.SCENE_SET:
        gpu, cam, opt = world(name)
        got = gpu.render_features(cam, opt, followed={"max_bounces": 8})
        assert_bits_equal(got, ffr.reference(oracle_lib, name, 8)[0], name)
        first = gpu.render_features(cam, opt)
        rays += 4 * W * H
        lost += int(round(float(((first[..., 0, 3] - got[..., 0, 3]) * 4).sum())))
        changed += int((first.view(np.uint32) != got.view(np.uint32)).any(axis=(2, 3)).sum())
    shares = ffr.shares(oracle_lib)
    print({k: round(v, 4) for k, v in shares.items()}, "escaped, from the device's coverage: %.4f" % (lost / rays))
    for key, least in ffr.SHARE_MIN.items():
        assert shares[key] >= least, (key, shares[key])
    assert lost / rays == shares["escaped"]
    assert changed * 4 / rays >= 0.25


DEVICE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding, scenes
from tests import features_follow_ref as ffr
W, H = ffr.WIDTH, ffr.HEIGHT
sc, cam, epsilon = ffr.scene("one_way")
gpu = binding.Scene(sc, device=0)
opt = scenes.options(W, H, 1, 1, epsilon=epsilon)
cams = ffr.view_cameras(cam)
side = torch.cuda.Stream(device=0)
checks = {}
for what, stream in (("current stream", torch.cuda.current_stream(0)), ("a side stream", side)):
    with torch.cuda.stream(stream):
        d_one = torch.full((H, W, 3, 4), -7.0, dtype=torch.float32, device="cuda:0")
        d_views = torch.full((3, H, W, 3, 4), -7.0, dtype=torch.float32, device="cuda:0")
        gpu.render_features_device(cam, opt, d_one.data_ptr(), stream.cuda_stream, followed={"max_bounces": 8})
        gpu.render_features_views_device(cams, opt, d_views.data_ptr(), stream.cuda_stream, followed={"max_bounces": 2})
        one, views = d_one.cpu().numpy(), d_views.cpu().numpy()  # (copies ordered on the same stream)
    checks["render_features_device, " + what] = (one, gpu.render_features(cam, opt, followed={"max_bounces": 8}))
    checks["render_features_views_device, " + what] = (views, gpu.render_features_views(cams, opt, followed={"max_bounces": 2}))
ok = True
for what, (got, want) in checks.items():
    same = bool((got.view(np.uint32) == want.view(np.uint32)).all())
    print("%s: %s" % (what, "bit-identical" if same else "DIFFERENT"))
    ok = ok and same
sys.exit(0 if ok else 1)
"""


def test_device_memory_forms():
    """The _device forms, on the caller's stream, equal the host forms bit for bit.  In a fresh interpreter in which torch opens the device
    first (torch cannot take the device over from the library in the same process)."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("bit-identical") == 4, r.stdout


# ---- frames ------------------------------------------------------------------------------------------------------------------------------

def test_complete_frame_previews_with_the_features_it_is_told(world):
    gpu, cam, _ = world("glass")
    opt = scenes.options(W, H, 4, 4, epsilon=1e-3)
    frame = binding.Frame(gpu, cam, opt, base_seed=77)
    try:
        image, _, info = frame.render()
        assert info["status"] == binding.PT_OK
        first = gpu.render_features(cam, opt)
        today, _ = frame.preview(denoise=True)
        assert_bits_equal(today, binding.denoise(image, first), "a frame starts with first-hit features")
        wants = {}
        for mb in (8, 1):  # (a preview, a change of the parameters, a preview: the cached features are dropped)
            frame.set_feature_params({"max_bounces": mb})
            feat = gpu.render_features(cam, opt, followed={"max_bounces": mb})
            wants[mb] = binding.denoise(image, feat)
            assert_bits_equal(frame.preview(denoise=True)[0], wants[mb], "%d bounces" % mb)
            assert_bits_equal(frame.preview_measured()[0], wants[mb], "%d bounces, measured form (a complete frame has no rated pixel)" % mb)
        assert not np.array_equal(wants[8], wants[1]) and not np.array_equal(wants[8], today)
        frame.set_feature_params(binding.FeatureParams(0, 0))
        assert_bits_equal(frame.preview(denoise=True)[0], today, "0 bounces")
        frame.set_feature_params({"max_bounces": 8})
        frame.set_feature_params(None)
        assert_bits_equal(frame.preview(denoise=True)[0], today, "NULL restores today's preview")
        with pytest.raises(binding.PtError):
            frame.set_feature_params({"max_bounces": 33})
        assert_bits_equal(frame.preview(denoise=True)[0], today, "a refused call changes nothing")
    finally:
        frame.close()


def test_stopped_frame_previews_as_the_masked_filter(world):
    gpu, cam, _ = world("one_way")
    opt = scenes.options(W, H, 8, 64, epsilon=1e-3)
    frame = binding.Frame(gpu, cam, opt, base_seed=78)
    try:
        frame.set_progressive(8, 1)
        assert frame.render()[2]["status"] == binding.PT_ERR_CANCELLED
        raw, samples = frame.preview()
        assert (samples > 0).any()
        zeros = np.zeros_like(raw)
        frame.set_feature_params({"max_bounces": 8})
        feat = gpu.render_features(cam, opt, followed={"max_bounces": 8})
        got, got_samples = frame.preview(denoise=True)
        # (pt_denoise_measured with a mask and a plane of zeros is the hole-aware filter of pt_frame_preview: include/pt_frame_variance.h)
        assert_bits_equal(got, binding.denoise_measured(raw, feat, zeros, mask=samples, params={"sigma_measured": 0.0}), "stopped frame, followed features")
        assert (got_samples == samples).all()
        assert_bits_equal(frame.preview_measured()[0], binding.denoise_measured(raw, feat, frame.variance(), mask=samples), "measured preview, followed features")
        frame.set_feature_params(None)
        assert_bits_equal(frame.preview(denoise=True)[0], binding.denoise_measured(raw, gpu.render_features(cam, opt), zeros, mask=samples, params={"sigma_measured": 0.0}),
                          "stopped frame, first-hit features again")
    finally:
        frame.close()


def test_view_frame_previews_with_followed_features(world):
    gpu, cam, _ = world("hall")
    opt = scenes.options(W, H, 2, 2, epsilon=1e-3)
    cams = ffr.view_cameras(cam)[:2]
    frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=[5, 6])
    try:
        images, _, info = frame.render()
        assert info["status"] == binding.PT_OK
        today, _ = frame.preview(denoise=True)
        assert_bits_equal(today, binding.denoise_views(images, gpu.render_features_views(cams, opt)), "a view frame starts with first-hit features")
        frame.set_feature_params({"max_bounces": 8})
        want = binding.denoise_views(images, gpu.render_features_views(cams, opt, followed={"max_bounces": 8}))
        assert_bits_equal(frame.preview(denoise=True)[0], want, "view frame, followed features")
        assert not np.array_equal(want, today)
        frame.set_feature_params(None)
        assert_bits_equal(frame.preview(denoise=True)[0], today, "view frame, NULL")
    finally:
        frame.close()


def test_cpp_api(tmp_path):
    """tests/cpp/features_test.cpp on the device: denoise(..., FeatureParams{0}) is denoise(...), FeatureParams{8} changes a frame that
    shows a mirror, max_bounces 33 throws."""
    from cpupathtrace_amd import build_host
    exe = str(tmp_path / "features_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "features_test.cpp")], exe, extra_flags=["-O1"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "FAILED" not in r.stdout and "skipped" not in r.stdout and r.stdout.count(": ok") == 9, r.stdout


# ---- bsdf_follow alone -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe():
    from tests import follow_probe
    p = follow_probe.Probe()
    assert p.device_count() >= 1
    return p


@pytest.mark.parametrize("epsilon", uc.EPSILONS)
def test_bsdf_follow_glass(probe, oracle_lib, epsilon):
    """The family and the engine states of tests/test_features_follow_cpu.py: the oracle's reflection where it reflects totally, a refracting state's ray where
    one of the 8 states refracts."""
    (rays, pos, nrm, ior), tir, outs, through = ffr.glass_oracle_answers(oracle_lib, epsilon)
    got, reflected = probe.bsdf_follow(1, 0, rays, pos, nrm, epsilon, ior)
    assert (reflected == tir).all()
    assert_bits_equal(got[tir], outs[0][tir], "total reflection")
    rest = np.nonzero(~tir)[0]
    has = through[:, rest].any(axis=0)
    sel = rest[has]
    assert len(sel) >= 0.85 * len(rest)
    assert_bits_equal(got[sel], outs[through[:, sel].argmax(axis=0), sel], "refraction")
    # and everywhere, the restatement
    assert_bits_equal(got, ffr.glass_follow(rays[:, 3:], pos, nrm, ior, epsilon)[0], "restatement")


@pytest.mark.parametrize("one_way", [0, 1])
def test_bsdf_follow_mirror(probe, oracle_lib, one_way):
    rays, pos, nrm, ior, states = uc.bsdf_propagate_family(4)
    for epsilon in uc.EPSILONS:
        want = oracle_lib.bsdf_propagate(2, one_way, rays, pos, nrm, epsilon, ior, states)[0]
        got, reflected = probe.bsdf_follow(2, one_way, rays, pos, nrm, epsilon, ior)
        assert_bits_equal(got, want, "mirror, one_way %d, eps %g" % (one_way, epsilon))
        passed = (ffr.dot32(rays[:, 3:], nrm) > 0) if one_way else np.zeros(len(rays), bool)
        assert (reflected == ~passed).all()


def test_bsdf_follow_odd_sizes(probe):
    """One case, one more than a workgroup: the guarded tail and the guard bands."""
    rays, pos, nrm, ior, _ = uc.bsdf_propagate_family(5, n=600)
    for n in (1, 257):
        got, _ = probe.bsdf_follow(1, 0, rays[:n], pos[:n], nrm[:n], 1e-3, ior[:n])
        assert_bits_equal(got, ffr.glass_follow(rays[:n, 3:], pos[:n], nrm[:n], ior[:n], 1e-3)[0], "n = %d" % n)


# ---- quality -----------------------------------------------------------------------------------------------------------------------------

# relMSE(followed) <= R x relMSE(first-hit), over S (a primary ray's first hit is specular) and over the rest: the ratios tools/follow_sweep.py
# measured ON THE CPU with the restatement on the oracle's frames (profiles/follow_sweep.txt), widened by 10 % -- the frames are the same bits
# on both sides, so only the filters' fp32 differences need covering (the margin of DESIGN.md 4.16).
R = {"cornell": {"S": 0.2423, "rest": 0.9969}, "advanced": {"S": 0.0605, "rest": 0.9588}}


@pytest.mark.parametrize("name", ["cornell", "advanced"])
def test_quality(oracle_lib, name):
    q = ffr.QUALITY
    n = q["size"]
    sc, cam = ffr.quality_scene(name)
    gpu = binding.Scene(sc, device=0)
    try:
        noisy = gpu.process_job(cam, scenes.options(n, n, q["samples"], q["samples"], epsilon=q["epsilon"]), base_seed=q["seed"])
        truth = gpu.process_job(cam, scenes.options(n, n, q["truth_samples"], q["truth_samples"], epsilon=q["epsilon"]), base_seed=q["truth_seed"])
        opt = scenes.options(n, n, 1, 1, epsilon=q["epsilon"])
        first = binding.denoise(noisy, gpu.render_features(cam, opt))
        followed = binding.denoise(noisy, gpu.render_features(cam, opt, followed={"max_bounces": q["max_bounces"]}))
    finally:
        gpu.close()
    in_s = ffr.first_hit_specular(oracle_lib, sc, cam, n, n) > 0
    for what, where in (("S", in_s), ("rest", ~in_s)):
        rn, rf, ro = (ffr.relmse_on(x, truth, where) for x in (noisy, first, followed))
        print("%s, %s (%d pixels): relMSE noisy %.5g, first-hit %.5g, followed %.5g, ratio %.4f (bound %.4f)" % (name, what, where.sum(), rn, rf, ro, ro / rf, R[name][what] * 1.1))
        assert ro <= R[name][what] * 1.1 * rf, (name, what)
