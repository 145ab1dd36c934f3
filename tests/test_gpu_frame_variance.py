"""The variance map of a frame and its measured preview on the GPU (pt_frame_get_variance, pt_frame_preview_measured; binding.Frame.variance /
preview_measured): the map equals tests/denoise_measured_ref.py::pixel_variance on the oracle's samples bit for bit after
1, 2 and 3 passes, with one replica and with two; finished, untouched and uncovered pixels are zero; a complete frame's measured preview is
its denoised preview bit for bit; a stopped frame's is the restatement fed the oracle's map; the frame then finishes equal to process_job bit
for bit; and the quality of the measured preview against today's denoised preview on the sweep's two frames (tools/measured_sweep.py).
Every call is limited to whole passes, so nothing here depends on a clock."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from cpupathtrace_amd import binding, scenes
from tests import denoise_measured_ref as mr
from tests import noise_ref
from tests.test_gpu_denoise_units import _close
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("measured_sweep", os.path.join(ROOT, "tools", "measured_sweep.py"))
measured_sweep = importlib.util.module_from_spec(_spec)  # (the sweep's frames, truth and relMSE: one definition for the sweep and this test)
_spec.loader.exec_module(measured_sweep)

F = np.float32
SEED = 4711
QUANTUM = 16

# relMSE(measured preview) <= R x relMSE(existing denoised preview) on the sweep's frames: the ratio tools/measured_sweep.py measured on the
# CPU for the default sigma_measured = 16 (profiles/measured_sweep.txt: Cornell 0.5184, Box 0.9316), widened by 10 % -- the frames are the
# same bits on both sides, so only the filters' fp32 differences of order 1e-4 need covering.
R = {"cornell": 0.5184 * 1.1, "box": 0.9316 * 1.1}


def _pass(frame):
    frame.set_progressive(QUANTUM, 1)
    return frame.render()[2]


def _oracle_map(handle, cam, opt, samples):
    """The variance map the oracle's estimator gives for the unfinished pixels of `samples`, zeros elsewhere."""
    h, w = samples.shape
    ys, xs = np.nonzero(samples > 0)
    count, _, m2, accepted = noise_ref.batch_stats(handle, cam, opt, SEED, xs, ys, samples[ys, xs], binding.pixel_seed, binding.seed_to_state)
    assert not accepted.any(), "a pixel the device has not finished is not finished by the oracle's estimator"
    want = np.zeros((h, w, 4), F)
    want[ys, xs] = mr.pixel_variance(count, m2, noise_ref.stats_sample_count(opt))
    return want


@pytest.fixture(scope="module", params=[32, 64])
def world(request):
    """The Cornell box at min 8 / max 64 samples (batches of 2) on the GPU and in the oracle and -- computed once, never changed -- where a
    frame stands after 1, 2 and 3 passes of 16 samples: sample counts, raw preview, variance map, and the oracle's map."""
    side = request.param
    sc, cam = scenes.cornell_scene(side, side)
    opt = scenes.options(side, side, 8, 64)
    gpu = binding.Scene(sc, device=0)
    chk = oracle.Checker("oracle")
    h = chk.scene_create(sc)
    w = {"side": side, "sc": sc, "cam": cam, "opt": opt, "gpu": gpu, "oracle": h, "passes": []}
    try:
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        try:
            assert (frame.variance() == 0).all(), "before the first render every pixel is untouched"
            for _ in range(3):
                assert _pass(frame)["status"] == binding.PT_ERR_CANCELLED
                raw, samples = frame.preview()
                var = frame.variance()
                for a in (raw, samples, var):
                    a.setflags(write=False)
                w["passes"].append({"raw": raw, "samples": samples, "var": var, "want": _oracle_map(h, cam, opt, samples)})
        finally:
            frame.close()
        yield w
    finally:
        h.close()
        gpu.close()


def test_map_equals_the_oracle_bit_for_bit(world):
    for k, p in enumerate(world["passes"]):
        var, samples, want = p["var"], p["samples"], p["want"]
        what = "%d x %d after %d passes" % (world["side"], world["side"], k + 1)
        assert var.shape == samples.shape + (4,) and var.dtype == F
        unfinished = samples > 0
        assert (samples[unfinished] == (k + 1) * QUANTUM).all() and (samples != 0).all(), what
        rated = mr.rated(var)
        print("%s: %d unfinished pixels, %d rated, %d finished; v %g .. %g" % (what, unfinished.sum(), rated.sum(), (samples == -1).sum(),
                                                                                  var[rated][:, :3].min(), var[rated][:, :3].max()))
        assert unfinished.sum() >= 128 and (rated <= unfinished).all() and rated.sum() >= 0.9 * unfinished.sum(), what
        assert_bits_equal(var, want, what + ": the variance map against pixel_variance on the oracle's samples")
        assert (var[samples == -1] == 0).all(), what + ": finished pixels"
        assert (var[rated][:, 3] >= 2).all() and (var[rated][:, 3] <= (k + 1) * QUANTUM // 2).all(), what  # (batches of 2 collected samples)
    assert (world["passes"][0]["samples"] == -1).sum() < (world["passes"][2]["samples"] == -1).sum(), "pixels finish between the passes"


def test_two_replicas_and_uncovered_pixels(world):
    side, gpu, cam, opt = world["side"], world["gpu"], world["cam"], world["opt"]
    second = binding.Scene(world["sc"], device=0)
    try:
        frame = binding.Frame([gpu, second], cam, opt, base_seed=SEED)
        try:
            for k in range(3):
                _pass(frame)
                assert_bits_equal(frame.variance(), world["passes"][k]["var"], "two replicas after %d passes" % (k + 1))
            rgba, samples = frame.preview_measured()
            one = binding.Frame(gpu, cam, opt, base_seed=SEED)
            try:
                for _ in range(3):
                    _pass(one)
                want, want_samples = one.preview_measured()
            finally:
                one.close()
            assert_bits_equal(rgba, want, "the measured preview of two replicas")
            assert_bits_equal(samples, want_samples, "its sample counts")
        finally:
            frame.close()
    finally:
        second.close()
    # a frame over all tiles but the last: the same values on its tiles, zeros outside them
    tiles = binding.job_tiles(side, side)[:-1]
    covered = np.zeros((side, side), bool)
    for t in tiles:
        covered[t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]] = True
    assert 0 < (~covered).sum() < side * side
    frame = binding.Frame(gpu, cam, opt, base_seed=SEED, tiles=tiles)
    try:
        _pass(frame)
        part = frame.variance()
        assert (part[~covered] == 0).all()
        assert_bits_equal(part[covered], world["passes"][0]["var"][covered], "a frame over all tiles but one")
    finally:
        frame.close()


def test_measured_preview(world):
    """Stopped: the restatement fed the raw preview, the device's features and the ORACLE's map.  Then the frame goes on as if nobody had
    looked, and complete it previews as the plain denoised preview does, with a map of zeros."""
    gpu, cam, opt = world["gpu"], world["cam"], world["opt"]
    feat = gpu.render_features(cam, opt)
    frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
    try:
        for k in range(2):
            _pass(frame)
        p = world["passes"][1]
        for params in (None, {"sigma_measured": 0.0}, {"sigma_measured": 2.0, "iterations": 3}):
            got, samples = frame.preview_measured(params)
            assert_bits_equal(samples, p["samples"], "the sample counts are the raw preview's")
            kw = dict(mr.DEFAULTS, **(params or {}))
            want = mr.denoise(p["raw"], feat, p["want"], p["samples"], **kw)
            e = _close(got, want, "%d x %d, measured preview %s" % (world["side"], world["side"], params))
            print("%d x %d, %s: largest difference %.3g of the largest value" % (world["side"], world["side"], params, e))
        plain, _ = frame.preview(denoise=True)
        assert (got != plain).any(), "the plane is read"
        assert_bits_equal(frame.variance(), p["var"], "the preview changes nothing")
        frame.set_progressive(0)
        image, tile_done, info = frame.render()
        assert info["status"] == binding.PT_OK and tile_done.all() and frame.done
        assert_bits_equal(image, gpu.process_job(cam, opt, base_seed=SEED), "the finished frame against process_job")
        assert (frame.variance() == 0).all(), "a complete frame has no rated pixel"
        done, samples = frame.preview_measured()
        assert (samples == -1).all()
        assert_bits_equal(done, frame.preview(denoise=True)[0], "a complete frame's measured preview against its denoised preview")
        assert_bits_equal(done, binding.denoise(image, feat), "... which is pt_denoise of the image")
    finally:
        frame.close()


def test_denoise_measured_entry_point(world):
    """pt_denoise_measured on host arrays: the stopped frame's raw preview with its own map is pt_frame_preview_measured; without a mask and
    with a map of zeros it is pt_denoise."""
    gpu, cam, opt = world["gpu"], world["cam"], world["opt"]
    feat = gpu.render_features(cam, opt)
    p = world["passes"][1]
    frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
    try:
        for k in range(2):
            _pass(frame)
        want, _ = frame.preview_measured()
    finally:
        frame.close()
    assert_bits_equal(binding.denoise_measured(p["raw"], feat, p["var"], mask=p["samples"]), want, "pt_denoise_measured against the frame's preview")
    assert_bits_equal(binding.denoise_measured(p["raw"], feat, np.zeros_like(p["var"])), binding.denoise(p["raw"], feat), "a map of zeros, no mask: pt_denoise")


DEVICE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding, scenes
torch.zeros(1, device="cuda:0")
sc, cam = scenes.cornell_scene(61, 47)
gpu = binding.Scene(sc, device=0)
opt = scenes.options(61, 47, 8, 64)
feat = gpu.render_features(cam, opt)
frame = binding.Frame(gpu, cam, opt, base_seed=5)
frame.set_progressive(16, 1)
frame.render()
raw, samples = frame.preview()
var = frame.variance()
frame.close()
stream = torch.cuda.current_stream(0).cuda_stream
d_img, d_feat, d_var, d_mask = (torch.from_numpy(a).to("cuda:0") for a in (raw, feat, var, samples))
d_out = torch.empty_like(d_img)
checks = {}
binding.denoise_measured_device(d_img.data_ptr(), d_feat.data_ptr(), d_var.data_ptr(), 61, 47, d_out.data_ptr(), d_mask.data_ptr(), stream)
checks["denoise_measured_device with a mask"] = (d_out.cpu().numpy(), binding.denoise_measured(raw, feat, var, mask=samples))
params = {"iterations": 2, "sigma_measured": 3.0}
binding.denoise_measured_device(d_img.data_ptr(), d_feat.data_ptr(), d_var.data_ptr(), 61, 47, d_out.data_ptr(), 0, stream, params=params)
checks["denoise_measured_device without a mask, with parameters"] = (d_out.cpu().numpy(), binding.denoise_measured(raw, feat, var, params=params))
binding.denoise_measured_device(d_img.data_ptr(), d_feat.data_ptr(), d_var.data_ptr(), 61, 47, d_img.data_ptr(), 0, stream, params=params)
checks["denoise_measured_device in place"] = (d_img.cpu().numpy(), checks["denoise_measured_device without a mask, with parameters"][1])
ok = (var[..., 3] >= 2).sum() >= 1000
for what, (got, want) in checks.items():
    same = bool((got.view(np.uint32) == want.view(np.uint32)).all())
    print("%s: %s" % (what, "bit-identical" if same else "DIFFERENT"))
    ok = ok and same
sys.exit(0 if ok else 1)
"""


def test_device_memory_form():
    """pt_denoise_measured_device (also in place) on torch tensors equals the host form bit for bit.  In a fresh interpreter in which torch
    opens the device first, as tests/test_gpu_denoise.py::test_device_memory_forms."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("bit-identical") == 3, r.stdout


@pytest.mark.parametrize("name", ["cornell", "box"])
def test_quality(name):
    """The sweep's frame on the device: relMSE against 1024 spp of the measured preview at its defaults against today's denoised preview
    at its defaults.  DESIGN.md 4.16 has the measured values."""
    sc, cam, opt = measured_sweep.scene_of(name)
    fr = measured_sweep.FRAME
    n = fr["size"]
    gpu = binding.Scene(sc, device=0)
    try:
        truth = gpu.process_job(cam, scenes.options(n, n, fr["truth_samples"], fr["truth_samples"]), base_seed=fr["truth_seed"])
        frame = binding.Frame(gpu, cam, opt, base_seed=fr["seed"])
        try:
            frame.set_progressive(fr["quantum"], 1)
            assert frame.render()[2]["status"] == binding.PT_ERR_CANCELLED
            raw, samples = frame.preview()
            var = frame.variance()
            existing, _ = frame.preview(denoise=True)
            measured, _ = frame.preview_measured()
        finally:
            frame.close()
    finally:
        gpu.close()
    unfinished = samples > 0
    assert (samples[unfinished] == fr["quantum"]).all() and mr.rated(var)[unfinished].all(), "every unfinished pixel is rated after the first pass"
    assert unfinished.mean() >= 0.99
    rr, re, rm = (measured_sweep.relmse(a, truth) for a in (raw, existing, measured))
    means = [a[..., :3].astype(np.float64).mean(axis=(0, 1)) for a in (raw, existing, measured, truth)]
    print("%s: relMSE raw %.5g, existing denoised preview %.5g, measured preview %.5g (ratio %.4f, bound %.4f); channel means raw %s existing %s measured %s 1024 spp %s" % (
        name, rr, re, rm, rm / re, R[name], *means))
    assert rm <= R[name] * re
