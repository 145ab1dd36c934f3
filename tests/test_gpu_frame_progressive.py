"""Progressive frames on the GPU (pt_frame_set_progressive, pt_frame_get_progress; binding.Frame.set_progressive / progress;
FrameRender::setProgressive): a frame rendered in passes of a sample quantum per pixel.  However the passes were cut -- any quantum, a
quantum changed between calls, stops inside a pass -- the finished frame equals process_job / process_views bit for bit and draws exactly
the samples of the uninterrupted render; after every pass every unfinished pixel has exactly the pass's sample count, also in a frame
with more pixels than the device has stream slots and in the later views of a batch; its preview is the oracle's running mean; a stop
inside a pass loses no sample.  Every case but the budgeted one limits a call to whole passes (max_passes_per_call), so nothing here
depends on a clock."""
import os
import subprocess
import threading

import numpy as np
import pytest

import oracle
from cpupathtrace_amd import binding, build_host, scenes
from tests import preview_ref
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 4711
MAX_CALLS = 400


def _views(cam, n):
    """n cameras around `cam`: pinhole, circular and hexagonal aperture in turn, each from a different place (as tests/test_gpu_views_frame.py)."""
    out = []
    for v in range(n):
        c = dict(cam)
        c["origin"] = (cam["origin"][0] + 0.07 * v, cam["origin"][1] + 0.03 * (v % 3), cam["origin"][2] - 0.02 * v)
        kind = v % 3
        c["aperture_kind"] = kind
        c["aperture_width"] = c["aperture_height"] = 0.0 if kind == 0 else 0.04 + 0.01 * v
        c["hex_ratio"] = 0.35 if kind == 2 else 0.0
        c["focal_plane_dist"] = 0.0 if kind == 0 else 3.0 + 0.1 * v
        out.append(c)
    return out


def _doubling():
    """1, 1, 2, 4, 8, ...: every pixel at 1, 2, 4, 8, 16 ... samples"""
    yield 1
    q = 1
    while True:
        yield q
        q *= 2


def _constant(q):
    while True:
        yield q


def _scene(name):
    if name == "box":
        return scenes.box_scene()
    if name == "cornell":
        return scenes.cornell_scene(256, 256)
    return scenes.dragon_box_scene(*scenes.bumpy_sphere_mesh(300, 300, scenes.DRAGON_BOX_TRANSFORM))  # 179,400 triangles


def _run_passes(frame, quanta, opt, what):
    """One pass per call, the quantum of every call from `quanta`; checks the pass contract after every call.  Returns the calls' infos."""
    infos, target = [], 0
    for q in quanta:
        assert len(infos) < MAX_CALLS, what
        frame.set_progressive(q, 1)
        _, tile_done, info = frame.render()
        infos.append(info)
        target += q
        pr = frame.progress()
        assert pr["samples_lost"] == 0 and pr["pass_in_progress"] == 0 and pr["passes_completed"] == len(infos) and pr["target"] == target, (what, pr)
        fi = info["frame"]
        assert fi["streams_untouched"] == 0, (what, fi)
        if info["status"] == binding.PT_OK:
            assert tile_done.all() and frame.done, what
            break
        assert info["status"] == binding.PT_ERR_CANCELLED
        # every unfinished pixel has exactly the pass's sample count
        assert pr["min_samples"] == pr["max_samples"] == target, (what, pr)
        assert pr["streams_at_target"] == fi["streams_parked"] == fi["streams_total"] - fi["streams_finished"], (what, pr, fi)
        assert fi["samples_carried"] == target * fi["streams_parked"], (what, fi)
        assert target < opt["max_sample_count"], (what, "unfinished pixels at or beyond max_sample_count")
    return infos


@pytest.mark.parametrize("name", ["box", "cornell", "mesh179k"])
def test_bit_exact_for_any_slicing(name):
    sc, cam = _scene(name)
    gpu = binding.Scene(sc, device=0)
    try:
        for lo, hi in ((16, 16), (16, 64), (0, 24)):
            opt = scenes.options(256, 256, lo, hi)
            full, full_stats = gpu.process_job(cam, opt, base_seed=SEED, want_stats=True)
            schedules = [("q1", _constant(1)), ("q3", _constant(3)), ("q16", _constant(16)), ("q%d" % (hi + 1), _constant(hi + 1)), ("doubling", _doubling())]
            for label, quanta in schedules:
                what = "%s (%d, %d) %s" % (name, lo, hi, label)
                frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
                try:
                    infos = _run_passes(frame, quanta, opt, what)
                    assert_bits_equal(frame.image, full, what)
                    drawn = sum(st["samples"] for info in infos for st in info["stats"])
                    print("%s: %d passes, %d samples" % (what, len(infos), drawn))
                    assert drawn == full_stats["samples"], (what, drawn, full_stats["samples"])
                    if label == "q%d" % (hi + 1):
                        assert len(infos) == 1, what
                    if label == "q3" and lo == hi:
                        assert len(infos) == -(-hi // 3), (what, len(infos))  # (max is no multiple of 3: the last pass is a short one)
                finally:
                    frame.close()
    finally:
        gpu.close()


def test_even_advance_on_a_frame_larger_than_the_slot_pool():
    sc, cam = scenes.box_scene()
    gpu = binding.Scene(sc, device=0)
    try:
        width, height = 2048, 1024
        for _ in range(4):
            # control: today's behaviour -- a plain frame stopped after its first slice has pixels no stream slot has reached
            opt = scenes.options(width, height, 64, 64)
            plain = binding.Frame(gpu, cam, opt, base_seed=SEED)
            try:
                plain.render(budget_ms=30)
                untouched = plain.info()["streams_untouched"]
            finally:
                plain.close()
            print("%d x %d: a stopped plain frame leaves %d streams untouched" % (width, height, untouched))
            if untouched > 0:
                break
            height *= 2  # (a device that holds the whole frame in its slots)
        assert untouched > 0
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        try:
            frame.set_progressive(4, 1)
            for target in (4, 8):
                _, _, info = frame.render()
                assert info["status"] == binding.PT_ERR_CANCELLED
                rgba, samples = frame.preview()
                assert (samples == target).all(), (target, np.unique(samples))
                pr = frame.progress()
                assert pr["min_samples"] == pr["max_samples"] == target and pr["samples_lost"] == 0, pr
                assert pr["streams_at_target"] == width * height
                fi = frame.info()
                assert fi["streams_untouched"] == 0 and fi["streams_parked"] == width * height
                print("pass to %d: %.1f ms kernel, park storage %.2f GB" % (target, sum(st["kernel_ms"] for st in info["stats"]), fi["park_bytes"] / 1e9))
        finally:
            frame.close()
    finally:
        gpu.close()


def test_preview_values():
    sc, cam = scenes.box_scene()
    opt = scenes.options(256, 256, 64, 64)
    gpu = binding.Scene(sc, device=0)
    chk = oracle.Checker("oracle")
    h = chk.scene_create(sc)
    try:
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        try:
            frame.set_progressive(4, 1)
            features = gpu.render_features(cam, opt)
            ys, xs = np.mgrid[0:256, 0:256]
            xs, ys = xs.ravel(), ys.ravel()
            for k in (1, 2, 3):
                frame.render()
                if k == 2:
                    continue
                raw, samples = frame.preview()
                assert (samples == 4 * k).all()
                want = preview_ref.raw_preview(h, cam, opt, SEED, xs, ys, samples[ys, xs], binding.pixel_seed, binding.seed_to_state)
                assert_bits_equal(raw[ys, xs], want, "raw preview after pass %d against the oracle's running mean" % k)
                clean, samples2 = frame.preview(denoise=True)
                assert (samples2 == samples).all()
                assert_bits_equal(clean, binding.denoise(raw, features), "denoised preview after pass %d" % k)
        finally:
            frame.close()
    finally:
        h.close()
        gpu.close()


def test_stops_inside_a_pass_lose_nothing():
    sc, cam = scenes.cornell_scene(1024, 1024)
    opt = scenes.options(1024, 1024, 16, 64)
    quantum = 8
    gpu = binding.Scene(sc, device=0)
    try:
        full = gpu.process_job(cam, opt, base_seed=SEED)
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        try:
            frame.set_progressive(quantum, 0)
            budget, calls, cut_short, cancelled = 3.0, 0, 0, False
            while not frame.done:
                assert calls < MAX_CALLS
                if calls == 3:
                    # once by the cancel flag, from another thread
                    control = binding.RenderControl()
                    timer = threading.Timer(0.03, control.cancel)
                    timer.start()
                    try:
                        _, _, info = frame.render(control=control)
                    finally:
                        timer.cancel()
                        timer.join()
                    cancelled = True
                else:
                    _, _, info = frame.render(budget_ms=budget)
                    budget = min(budget * 1.5, 4000.0)
                calls += 1
                pr = frame.progress()
                fi = info["frame"]
                assert pr["samples_lost"] == 0, pr
                cut_short += pr["pass_in_progress"]
                if info["status"] == binding.PT_ERR_CANCELLED:
                    assert pr["min_samples"] >= pr["target"] - quantum, pr
                    assert pr["max_samples"] <= pr["target"], pr
                    assert pr["target"] == quantum * (pr["passes_completed"] + pr["pass_in_progress"]), pr
                    assert fi["samples_carried"] >= pr["min_samples"] * (fi["streams_total"] - fi["streams_finished"]), (pr, fi)
            print("%d calls, %d ended inside a pass, cancel used: %s; %s" % (calls, cut_short, cancelled, frame.progress()))
            assert_bits_equal(frame.image, full, "a progressive frame stopped inside its passes")
        finally:
            frame.close()
    finally:
        gpu.close()


def test_view_frames():
    sc, cam = scenes.box_scene()
    opt = scenes.options(512, 512, 16, 16)
    cams, seeds = _views(cam, 6), [11, 2024, 77, 9001, 123456789012, 5]
    gpu = binding.Scene(sc, device=0)
    try:
        frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=seeds)
        try:
            frame.set_progressive(2, 1)
            _, _, info = frame.render()
            assert info["status"] == binding.PT_ERR_CANCELLED
            _, samples = frame.preview()
            assert samples.shape == (6, 512, 512)
            for v in range(6):
                assert (samples[v] == 2).all(), (v, np.unique(samples[v]))
            frame.set_progressive(2, 0)
            _, tile_done, info = frame.render()
            assert info["status"] == binding.PT_OK and tile_done.all()
            assert frame.progress()["passes_completed"] == 8
            assert_bits_equal(frame.image, gpu.process_views(cams, opt, base_seeds=seeds), "a progressive view frame")
        finally:
            frame.close()
    finally:
        gpu.close()


def test_two_replicas_on_one_device():
    sc, cam = scenes.box_scene()
    opt = scenes.options(768, 512, 8, 32)
    replicas = [binding.Scene(sc, device=0), binding.Scene(sc, device=0)]
    try:
        images = []
        for scene_list in (replicas[:1], replicas):
            frame = binding.Frame(scene_list, cam, opt, base_seed=SEED)
            try:
                infos = _run_passes(frame, _constant(5), opt, "%d replicas" % len(scene_list))
                assert all(st["launches"] <= 1 for info in infos for st in info["stats"]), "one pass is one launch per replica"
                images.append(frame.image.copy())
            finally:
                frame.close()
        assert_bits_equal(images[1], images[0], "two replicas against one")
        assert_bits_equal(images[0], replicas[0].process_job(cam, opt, base_seed=SEED), "a progressive frame on one replica")
    finally:
        for r in replicas:
            r.close()


def test_mode_off_again():
    sc, cam = scenes.cornell_scene(512, 512)
    opt = scenes.options(512, 512, 16, 64)
    gpu = binding.Scene(sc, device=0)
    try:
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        try:
            frame.set_progressive(4, 1)
            frame.render()
            frame.render()
            assert frame.progress()["passes_completed"] == 2
            frame.set_progressive(0, 0)
            launches = frame.info()["launches"]
            _, tile_done, info = frame.render()
            assert info["status"] == binding.PT_OK and tile_done.all() and frame.done
            assert frame.info()["launches"] == launches + 1, "a plain frame finishes in one launch"
            assert frame.progress()["quantum"] == 0
            assert_bits_equal(frame.image, gpu.process_job(cam, opt, base_seed=SEED), "progressive, then plain")
        finally:
            frame.close()
    finally:
        gpu.close()


def test_cpp_frame_progressive(tmp_path):
    exe = str(tmp_path / "frame_progressive_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "frame_progressive_test.cpp")], exe, extra_flags=["-O1"])
    path = [build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]
    r = subprocess.run([exe], env=dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(path)), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[ OK ]") == 5, r.stdout
