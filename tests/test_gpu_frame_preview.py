"""The preview of an unfinished frame on the GPU (pt_frame_preview, binding.Frame.preview, FrameRender::preview): the sample classes match
pt_frame_info, finished pixels are the frame's, parked ones are the oracle's running mean bit for bit, a preview changes nothing the frame
does, the denoised preview of a complete frame is process_job(allow_bias=True), and the device's hole-aware filter matches
tests/preview_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from cpupathtrace_amd import binding, build_host, scenes
from tests import denoise_ref, preview_ref
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 4711
MAX_CALLS = 60


def _lit_room(n_point_lights):
    """A closed room with Lambertian, glass and mirror objects, point lights and two emitters (12 lights: the 64-bit slot word)."""
    sb = scenes.SceneBuilder()
    sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), sb.material((0.75, 0.7, 0.65, 1.0)))
    sb.sphere((0.35, -0.6, 0.1), 0.35, sb.material((1, 1, 1, 1), 1.5, bsdf=scenes.BSDF_GLASS))
    sb.sphere((-0.45, -0.7, -0.3), 0.28, sb.material((0.9, 0.9, 1.0, 1), bsdf=scenes.BSDF_MIRROR))
    sb.triangles(scenes.make_plane((-0.25, 0.97, -0.25), (0.25, 0.97, 0.25)), sb.material((1, 1, 1, 1), 1.0, (4, 3.5, 3, 1)), cull=True)
    sb.sphere((-0.6, 0.4, 0.5), 0.1, sb.material((1, 1, 1, 1), 1.0, (1, 2, 4, 1)))
    for k in range(n_point_lights):
        a = 2.0 * np.pi * k / max(n_point_lights, 1)
        sb.point_light((0.7 * np.cos(a), 0.3 + 0.05 * k, 0.7 * np.sin(a)), (0.2 + 0.05 * k, 0.3, 0.5 - 0.02 * k, 1.0))
    return sb.build(), scenes.camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0)


def _slice_until(frame, want, budget_ms=20.0, grow=1.0):
    """Budgeted slices until want(info) holds (at most MAX_CALLS); returns the frame's info.  Each slice's budget is the last one's times
    `grow` (up to 2 s): the budget counts from the call's start, so on a busy host a short one can end every call before its launch has
    resumed the parked pixels."""
    for _ in range(MAX_CALLS):
        fi = frame.info()
        if want(fi):
            return fi
        assert not frame.done, "the frame finished before the state the test needs: %s" % fi
        frame.render(budget_ms=budget_ms)
        budget_ms = min(budget_ms * grow, 2000.0)
    fi = frame.info()
    assert want(fi), "no slice of %d left the state the test needs: %s" % (MAX_CALLS, fi)
    return fi


def _parked(fi):
    """Parked pixels that have taken several samples each on average (a first slice often parks every pixel after one)."""
    return fi["streams_parked"] >= 256 and fi["samples_carried"] >= 3 * fi["streams_parked"]


def _check_classes(frame, rgba, samples, fi, what):
    finished, parked, holes = samples == -1, samples >= 1, samples == 0
    assert int(finished.sum()) == fi["streams_finished"], what
    assert int(parked.sum()) == fi["streams_parked"], what
    assert int(holes.sum()) == fi["streams_untouched"], what
    assert (samples >= -1).all()
    assert int(samples[parked].astype(np.int64).sum()) == fi["samples_carried"], what
    assert_bits_equal(rgba[finished], frame.image[finished], what + ": finished pixels")
    assert (rgba[holes] == 0).all(), what + ": holes"


def _check_parked_against_oracle(sc, cam, opt, rgba, samples, what, n=256, seed=SEED):
    ys, xs = np.nonzero(samples >= 1)
    assert len(xs) >= n, "%s: only %d parked pixels" % (what, len(xs))
    pick = np.random.default_rng(len(xs)).choice(len(xs), n, replace=False)
    xs, ys = xs[pick], ys[pick]
    chk = oracle.Checker("oracle")
    h = chk.scene_create(sc)
    try:
        want = preview_ref.raw_preview(h, cam, opt, seed, xs, ys, samples[ys, xs], binding.pixel_seed, binding.seed_to_state)
    finally:
        h.close()
    assert_bits_equal(rgba[ys, xs], want, what + ": parked pixels against the oracle's running mean")


@pytest.fixture(scope="module")
def box():
    sc, cam = scenes.box_scene()
    gpu = binding.Scene(sc, device=0)
    yield sc, cam, gpu
    gpu.close()


def test_fresh_frame_is_all_holes(box):
    _, cam, gpu = box
    frame = binding.Frame(gpu, cam, scenes.options(320, 200, 8, 8), base_seed=SEED)
    try:
        for denoise in (None, True):
            rgba, samples = frame.preview(denoise=denoise)
            assert rgba.shape == (200, 320, 4) and samples.shape == (200, 320)
            assert (rgba == 0).all() and (samples == 0).all()
        assert frame.info()["launches"] == 0
    finally:
        frame.close()


@pytest.mark.parametrize("name", ["box", "room12", "mesh", "adaptive"])
def test_after_stops(box, name):
    if name == "box":
        sc, cam, _ = box
        opt = scenes.options(2048, 2048, 32, 32)
    elif name == "mesh":
        sc, cam = scenes.dragon_box_scene(*scenes.bumpy_sphere_mesh(200, 200, scenes.DRAGON_BOX_TRANSFORM))
        opt = scenes.options(2048, 2048, 16, 16)
    else:
        sc, cam = _lit_room(12 if name == "room12" else 2)
        opt = scenes.options(2048, 2048, 16, 64) if name == "adaptive" else scenes.options(2048, 2048, 16, 16)
    gpu = box[2] if name == "box" else binding.Scene(sc, device=0)
    try:
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        try:
            fi = _slice_until(frame, _parked, budget_ms=20.0, grow=2.0)
            rgba, samples = frame.preview()
            print("%s: %s" % (name, fi))
            _check_classes(frame, rgba, samples, fi, name)
            _check_parked_against_oracle(sc, cam, opt, rgba, samples, name)
        finally:
            frame.close()
    finally:
        if name != "box":
            gpu.close()


def test_across_slices_and_no_side_effects(box):
    _, cam, gpu = box
    opt = scenes.options(2048, 2048, 16, 16)
    full = gpu.process_job(cam, opt, base_seed=SEED)
    frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
    try:
        prev_rgba, prev_samples = frame.preview()
        calls = 0
        while not frame.done:
            assert calls < MAX_CALLS
            frame.render(budget_ms=50)
            calls += 1
            rgba, samples = frame.preview()
            frame.preview(denoise=True)
            was_parked, was_finished = prev_samples >= 1, prev_samples == -1
            assert ((samples[was_parked] == -1) | (samples[was_parked] >= prev_samples[was_parked])).all(), "a parked pixel lost samples"
            assert (samples[was_finished] == -1).all()
            assert_bits_equal(rgba[was_finished], prev_rgba[was_finished], "a finished pixel kept its bits")
            prev_rgba, prev_samples = rgba, samples
        assert calls >= 2
        assert_bits_equal(frame.image, full, "a frame previewed after every slice")
    finally:
        frame.close()


def test_complete_frame(box):
    _, cam, gpu = box
    opt = scenes.options(512, 384, 16, 16)
    frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
    try:
        frame.render()
        assert frame.done
        rgba, samples = frame.preview()
        assert_bits_equal(rgba, frame.image, "the preview of a complete frame")
        assert (samples == -1).all()
        clean, samples = frame.preview(denoise=True)
        assert (samples == -1).all()
        assert_bits_equal(clean, gpu.process_job(cam, opt, base_seed=SEED, allow_bias=True), "the denoised preview of a complete frame")
        params = {"iterations": 3, "sigma_luminance": 4.0, "sigma_normal": 64.0, "sigma_depth": 2.0}
        assert_bits_equal(frame.preview(denoise=params)[0], binding.denoise(frame.image, gpu.render_features(cam, opt), params=params),
                          "the denoised preview with parameters")
    finally:
        frame.close()


def test_two_replicas_on_one_device(box):
    sc, cam, _ = box
    opt = scenes.options(2048, 2048, 32, 32)
    replicas = [binding.Scene(sc, device=0), binding.Scene(sc, device=0)]
    try:
        frame = binding.Frame(replicas, cam, opt, base_seed=SEED)
        try:
            fi = _slice_until(frame, _parked, budget_ms=20.0, grow=2.0)
            rgba, samples = frame.preview()
            print("two replicas: %s" % fi)
            _check_classes(frame, rgba, samples, fi, "two replicas")
            _check_parked_against_oracle(sc, cam, opt, rgba, samples, "two replicas")
            # both replicas' tiles hold parked pixels
            owner = np.zeros(samples.shape, np.int32)
            for k, t in enumerate(frame.tiles):
                owner[t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]] = k % 2
            parked = samples >= 1
            assert parked[owner == 0].any() and parked[owner == 1].any()
            frame.render()
            assert_bits_equal(frame.preview()[0], binding.process_job_multi(replicas, cam, opt, base_seed=SEED), "two replicas, complete")
        finally:
            frame.close()
    finally:
        for r in replicas:
            r.close()


def test_holes_match_the_restatement(box):
    _, cam, gpu = box
    opt = scenes.options(2048, 2048, 64, 64)
    frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
    try:
        fi = _slice_until(frame, lambda i: i["streams_parked"] > 0 and i["streams_untouched"] > 0, grow=1.5)
        raw, samples = frame.preview()
        got, samples2 = frame.preview(denoise=True)
        assert (samples2 == samples).all()
        print("holes: %s" % fi)
        want = preview_ref.denoise(raw, gpu.render_features(cam, opt), samples, **denoise_ref.DEFAULTS)
        diff = np.abs(got.astype(np.float64) - want)
        print("largest difference %.3g" % np.nanmax(diff))
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)
        holes = samples == 0
        filled = got[holes, 3] == 1.0
        assert ((got[holes][~filled]) == 0).all()
        assert filled.any()
    finally:
        frame.close()


@pytest.mark.parametrize("name", ["cornell", "box"])
def test_denoised_preview_is_closer(name):
    sc, cam = scenes.cornell_scene(256, 256) if name == "cornell" else scenes.box_scene()
    opt = scenes.options(256, 256, 1024, 1024)
    gpu = binding.Scene(sc, device=0)
    try:
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        try:
            def enough(fi):
                if fi["streams_parked"] == 0:
                    return False
                return np.median(frame.preview()[1]) >= 8
            _slice_until(frame, enough, budget_ms=3.0, grow=1.25)
            raw, samples = frame.preview()
            clean, _ = frame.preview(denoise=True)
            frame.render()
            ref = frame.image

            def relmse(x):
                x, g = x[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
                return float(np.mean((x - g) ** 2 / (g ** 2 + 0.01)))
            print("%s: median samples %d; relMSE raw %.4g, denoised %.4g" % (name, np.median(samples), relmse(raw), relmse(clean)))
            assert relmse(clean) <= 0.5 * relmse(raw)
        finally:
            frame.close()
    finally:
        gpu.close()


def test_cpp_frame_preview(tmp_path):
    exe = str(tmp_path / "frame_preview_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "frame_preview_test.cpp")], exe, extra_flags=["-O1"])
    path = [build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]
    r = subprocess.run([exe], env=dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(path)), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[ OK ]") == 6, r.stdout


def test_bad_arguments(box):
    _, cam, gpu = box
    frame = binding.Frame(gpu, cam, scenes.options(64, 48, 4, 4), base_seed=SEED)
    lib = binding.load()
    try:
        frame.render(budget_ms=1)
        out = np.zeros_like(frame.image)
        P = binding._ptr
        assert lib.pt_frame_preview(frame._h, None, None, P(out), None) == 1
        assert lib.pt_frame_preview(frame._h, P(frame.image), None, None, None) == 1
        assert lib.pt_frame_preview(None, P(frame.image), None, P(out), None) == 1
        bad = binding.DenoiseParams(11, 32.0, 128.0, 1.0)
        assert lib.pt_frame_preview(frame._h, P(frame.image), C.byref(bad), P(out), None) == 1
        assert lib.pt_frame_preview(frame._h, P(frame.image), None, P(out), None) == 0  # out_samples may be NULL
        with pytest.raises(ValueError):
            frame.preview(denoise={"iterationz": 2})
    finally:
        frame.close()
    with pytest.raises(ValueError):
        frame.preview()
