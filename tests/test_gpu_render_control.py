"""Cancellable and time-budgeted processJob on the GPU (pt_render_tiles_ctl): a stop ends the launch early and cleanly, every pixel it
wrote is bit-identical to the full render, the streams are accounted for, and the scene renders as a fresh one afterwards."""
import os
import subprocess
import time

import numpy as np
import pytest

from cpupathtrace_amd import binding, build_host, scenes
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 777


def _sentinel(opt):
    return np.full((opt["image_height"], opt["image_width"], 4), np.nan, np.float32)


def _check_partial(img, full, tiles, tile_done):
    """Finished tiles equal the full render; every pixel is either the NaN sentinel or the full render's."""
    for t, done in zip(tiles, tile_done):
        if done:
            assert_bits_equal(img[t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]], full[t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]], "finished tile")
    written = ~np.isnan(img).all(axis=2)
    assert_bits_equal(img[written], full[written], "written pixels")
    return int(written.sum())


@pytest.fixture(scope="module")
def box():
    sc, cam = scenes.box_scene()
    gpu = binding.Scene(sc, device=0)
    yield sc, cam, gpu
    gpu.close()


def test_budget_not_reached_is_the_full_render(box):
    _, cam, gpu = box
    opt = scenes.options(96, 64, 4, 16)
    full = gpu.process_job(cam, opt, base_seed=SEED)
    img, tile_done, info = gpu.process_job_controlled(cam, opt, base_seed=SEED, budget_ms=600000)
    assert info["status"] == binding.PT_OK and not info["cancelled"]
    assert tile_done.all()
    assert info["streams_abandoned"] == 0 and info["streams_unclaimed"] == 0 and info["streams_finished"] == 96 * 64
    assert info["drain_ms"] == 0.0
    assert info["stats"][0]["launches"] == 1
    assert_bits_equal(img, full, "controlled render without a stop")


def test_cancel_from_progress_callback(box):
    _, cam, gpu = box
    opt = scenes.options(2048, 2048, 16, 16)  # 4 M streams, several times the slots of the device: tiles finish one after another
    full = gpu.process_job(cam, opt, base_seed=SEED)
    control = binding.RenderControl()
    reports = []

    def progress(done, total):
        reports.append(done)
        if done == 1:
            control.cancel()

    tiles = binding.job_tiles(2048, 2048)
    img, tile_done, info = gpu.process_job_controlled(cam, opt, base_seed=SEED, progress=progress, control=control, image=_sentinel(opt))
    print("cancel from progress: %d of %d tiles, finished %d abandoned %d unclaimed %d, drain %.3f ms" % (
        tile_done.sum(), len(tiles), info["streams_finished"], info["streams_abandoned"], info["streams_unclaimed"], info["drain_ms"]))
    assert info["status"] == binding.PT_ERR_CANCELLED and info["cancelled"]
    assert 0 < tile_done.sum() < len(tiles)
    assert reports == list(range(1, len(reports) + 1)) and len(reports) == tile_done.sum()
    assert info["streams_finished"] + info["streams_abandoned"] + info["streams_unclaimed"] == 2048 * 2048
    written = _check_partial(img, full, tiles, tile_done)
    assert written == info["streams_finished"]
    assert info["drain_ms"] > 0.0


def test_budget_expires(box):
    _, cam, gpu = box
    opt = scenes.options(2048, 2048, 512, 512)
    t0 = time.perf_counter()
    full = gpu.process_job(cam, opt, base_seed=SEED)
    t_full = time.perf_counter() - t0
    assert t_full > 0.5, "the frame is meant to take well over half a second"
    budget_ms = 0.05 * t_full * 1e3
    t0 = time.perf_counter()
    img, tile_done, info = gpu.process_job_controlled(cam, opt, base_seed=SEED, budget_ms=budget_ms, image=_sentinel(opt))
    t_ctl = time.perf_counter() - t0
    print("budget %.1f ms of a %.1f ms frame: returned after %.1f ms, drain %.3f ms, %d tiles finished" % (
        budget_ms, t_full * 1e3, t_ctl * 1e3, info["drain_ms"], tile_done.sum()))
    assert info["status"] == binding.PT_ERR_CANCELLED
    assert t_ctl < 0.5 * t_full
    assert info["streams_finished"] + info["streams_abandoned"] + info["streams_unclaimed"] == 2048 * 2048
    _check_partial(img, full, binding.job_tiles(2048, 2048), tile_done)


def test_scene_is_reusable_after_a_cancel(box):
    sc, cam, gpu = box
    opt_big = scenes.options(2048, 2048, 16, 16)
    control = binding.RenderControl()
    _, _, info = gpu.process_job_controlled(cam, opt_big, base_seed=SEED, progress=lambda d, t: control.cancel(), control=control)
    assert info["cancelled"]
    fresh = binding.Scene(sc, device=0)
    try:
        opt = scenes.options(64, 48, 2, 8)
        got, st = gpu.process_job(cam, opt, base_seed=SEED, want_stats=True)  # (with statistics: the launch's stream check runs)
        assert_bits_equal(got, fresh.process_job(cam, opt, base_seed=SEED), "process_job after a cancel")
        assert st["launches"] == 1
        streams = binding.pixel_streams(np.array([3, 10, 40]), np.array([5, 20, 47]), np.array([11, 22, 33], np.uint64))
        streams["w"][1], streams["h"][1] = 6, 4
        a_img, a_states = gpu.process_item(cam, opt, streams)
        b_img, b_states = fresh.process_item(cam, opt, streams)
        assert_bits_equal(a_img, b_img, "process_item after a cancel")
        assert (a_states == b_states).all()
        rays = np.random.default_rng(5).uniform(-0.9, 0.9, (500, 6)).astype(np.float32)
        ta, oa = gpu.get_intersection(rays)
        tb, ob = fresh.get_intersection(rays)
        assert_bits_equal(ta, tb, "getIntersection after a cancel")
        assert (oa == ob).all()
        # the big frame itself, uncancelled, on both
        assert_bits_equal(gpu.process_job(cam, opt_big, base_seed=SEED), fresh.process_job(cam, opt_big, base_seed=SEED), "full frame after a cancel")
    finally:
        fresh.close()


def test_cancel_outside_the_call(box):
    _, cam, gpu = box
    opt = scenes.options(128, 128, 8, 8)
    full = gpu.process_job(cam, opt, base_seed=SEED)
    old = binding.RenderControl()
    old.cancel()
    # a control cancelled before the call stops it at once: nothing is written
    img, tile_done, info = gpu.process_job_controlled(cam, opt, base_seed=SEED, control=old, image=_sentinel(opt))
    assert info["cancelled"] and not tile_done.any() and np.isnan(img).all()
    assert info["streams_finished"] == 0 and info["streams_abandoned"] + info["streams_unclaimed"] == 128 * 128
    # a new control is not cancelled
    img, tile_done, info = gpu.process_job_controlled(cam, opt, base_seed=SEED, control=binding.RenderControl())
    assert info["status"] == binding.PT_OK and tile_done.all()
    assert_bits_equal(img, full, "new control after a cancelled one")
    # a cancel after PT_OK changes nothing that follows
    done = binding.RenderControl()
    img, _, info = gpu.process_job_controlled(cam, opt, base_seed=SEED, control=done)
    assert info["status"] == binding.PT_OK
    done.cancel()
    assert_bits_equal(gpu.process_job(cam, opt, base_seed=SEED), full, "process_job after a late cancel")
    img, tile_done, info = gpu.process_job_controlled(cam, opt, base_seed=SEED)
    assert info["status"] == binding.PT_OK and tile_done.all()
    assert_bits_equal(img, full, "controlled render after a late cancel")


def test_one_cancel_stops_two_replicas(box):
    sc, cam, _ = box
    opt = scenes.options(2048, 2048, 16, 16)
    replicas = [binding.Scene(sc, device=0), binding.Scene(sc, device=0)]
    try:
        full = binding.process_job_multi(replicas, cam, opt, base_seed=SEED)
        control = binding.RenderControl()

        def progress(done, total):
            if done == 1:
                control.cancel()

        tiles = binding.job_tiles(2048, 2048)
        img, tile_done, info = binding.process_job_controlled_multi(replicas, cam, opt, base_seed=SEED, progress=progress, control=control, image=_sentinel(opt))
        print("two replicas: %d of %d tiles, drain %.3f ms" % (tile_done.sum(), len(tiles), info["drain_ms"]))
        assert info["status"] == binding.PT_ERR_CANCELLED
        assert 0 < tile_done.sum() < len(tiles)
        assert info["streams_finished"] + info["streams_abandoned"] + info["streams_unclaimed"] == 2048 * 2048
        assert len(info["stats"]) == 2 and all(s["launches"] == 1 for s in info["stats"])
        # both replicas stopped: neither finished all of its own tiles
        k = np.arange(len(tiles))
        owner = (k % 64 + k // 64) % 2  # (64 tiles per grid row: dealt along the diagonals, pt_render_tiles_multi)
        assert all(not tile_done[owner == i].all() for i in (0, 1))
        _check_partial(img, full, tiles, tile_done)
    finally:
        for r in replicas:
            r.close()


def test_cpp_render_control(tmp_path):
    exe = str(tmp_path / "render_control_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "render_control_test.cpp")], exe, extra_flags=["-O1"])
    path = [build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]
    r = subprocess.run([exe], env=dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(path)), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[ OK ]") == 7, r.stdout
