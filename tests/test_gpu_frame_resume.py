"""Resumable frames on the GPU (pt_frame_*, binding.Frame, PathTrace/frame_render.h): a frame stopped by its budget or a cancel parks its
half-finished pixels and the next call resumes them; however it was sliced, the finished frame equals one uninterrupted process_job /
process_job_multi with the same seed bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build_host, scenes
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2718
MAX_CALLS = 60


def _lit_room(n_point_lights):
    """A closed room with Lambertian, glass and mirror objects, point lights and two emitters (12 lights: 14 light samples per vertex,
    the kernel with the 64-bit slot word)."""
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


def _cancel_after(n_tiles):
    """A control and a progress callback that cancels it once `n_tiles` tiles of the call have been reported."""
    control = binding.RenderControl()
    seen = []

    def progress(done, total):
        seen.append(done)
        if len(seen) == n_tiles:
            control.cancel()
    return control, progress


def _finish(frame, calls=None):
    """Render the rest of a frame without a stop; returns the image."""
    img, tile_done, info = frame.render()
    assert info["status"] == binding.PT_OK and tile_done.all() and frame.done
    if calls is not None:
        calls.append(info)
    return img


@pytest.fixture(scope="module")
def box():
    sc, cam = scenes.box_scene()
    gpu = binding.Scene(sc, device=0)
    yield sc, cam, gpu
    gpu.close()


def test_sliced_by_budget_until_done(box):
    _, cam, gpu = box
    opt = scenes.options(2048, 2048, 64, 64)
    full = gpu.process_job(cam, opt, base_seed=SEED)
    frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
    try:
        infos, restored = [], False
        while not frame.done:
            assert len(infos) < MAX_CALLS, "the frame did not finish in %d slices" % MAX_CALLS
            img, tile_done, info = frame.render(budget_ms=50)
            infos.append(info)
            fi = info["frame"]
            restored = restored or (fi["streams_parked"] > 0 and fi["samples_carried"] > 0)
        print("budget 50 ms: %d calls; parked per call %s" % (len(infos), [i["streams_abandoned"] for i in infos]))
        assert len(infos) >= 2, "the frame finished in one slice: nothing was resumed"
        assert all(i["status"] == binding.PT_ERR_CANCELLED for i in infos[:-1]) and infos[-1]["status"] == binding.PT_OK
        assert sum(i["streams_finished"] for i in infos) == 2048 * 2048
        assert restored, "no call left parked streams with samples: the restore path was not used"
        assert_bits_equal(img, full, "frame sliced by a 50 ms budget")
        # a complete frame returns PT_OK without a launch
        launches = frame.info()["launches"]
        _, tile_done, info = frame.render(budget_ms=50)
        assert info["status"] == binding.PT_OK and tile_done.all() and frame.info()["launches"] == launches
    finally:
        frame.close()


def test_adaptive_estimator_is_carried_over():
    desc, cam = _lit_room(2)
    gpu = binding.Scene(desc, device=0)
    try:
        opt = scenes.options(2048, 2048, 16, 64)  # (more streams than slots: tiles finish one after another, and a stop finds most pixels half-way)
        full = gpu.process_job(cam, opt, base_seed=SEED)
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        try:
            control, progress = _cancel_after(2)
            _, _, info = frame.render(progress=progress, control=control)
            fi = info["frame"]
            print("adaptive: %s" % fi)
            assert info["status"] == binding.PT_ERR_CANCELLED
            assert fi["streams_parked"] > 0 and fi["parked_with_candidates"] > 0, "no parked stream holds closed candidates"
            assert_bits_equal(_finish(frame), full, "adaptive frame resumed after a cancel")
        finally:
            frame.close()
    finally:
        gpu.close()


def test_cancel_before_the_first_call(box):
    _, cam, gpu = box
    opt = scenes.options(256, 192, 8, 8)
    full = gpu.process_job(cam, opt, base_seed=SEED)
    frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
    try:
        control = binding.RenderControl()
        control.cancel()
        img, tile_done, info = frame.render(control=control)
        fi = info["frame"]
        assert info["status"] == binding.PT_ERR_CANCELLED and not tile_done.any()
        assert info["streams_finished"] == 0 and fi["streams_finished"] == 0 and fi["streams_parked"] == 0
        assert fi["streams_untouched"] == 256 * 192
        assert (img == 0).all()
        assert_bits_equal(_finish(frame), full, "frame cancelled before its first call, then completed")
    finally:
        frame.close()


def _stop_and_resume(scenes_, cam, opt, want, what, cancel_after=1):
    frame = binding.Frame(scenes_, cam, opt, base_seed=SEED)
    try:
        control, progress = _cancel_after(cancel_after)
        _, tile_done, info = frame.render(progress=progress, control=control)
        assert info["status"] == binding.PT_ERR_CANCELLED and not tile_done.all()
        assert info["frame"]["streams_parked"] > 0, "%s: the stop parked nothing" % what
        assert_bits_equal(_finish(frame), want, what)
    finally:
        frame.close()


def test_wide_slot_word():
    desc, cam = _lit_room(12)
    gpu = binding.Scene(desc, device=0)
    try:
        opt = scenes.options(2048, 2048, 8, 8)
        _stop_and_resume(gpu, cam, opt, gpu.process_job(cam, opt, base_seed=SEED), "12 point lights (wide slot word)")
    finally:
        gpu.close()


def test_trees_in_hbm_and_in_lds(box):
    _, box_cam, box_gpu = box
    opt = scenes.options(2048, 2048, 16, 16)
    _stop_and_resume(box_gpu, box_cam, opt, box_gpu.process_job(box_cam, opt, base_seed=SEED), "Box (scene in LDS)")
    desc, cam = scenes.dragon_box_scene(*scenes.bumpy_sphere_mesh(200, 200, scenes.DRAGON_BOX_TRANSFORM))
    gpu = binding.Scene(desc, device=0)
    try:
        opt = scenes.options(2048, 2048, 8, 8)
        _stop_and_resume(gpu, cam, opt, gpu.process_job(cam, opt, base_seed=SEED), "80 K triangle mesh (tree in HBM)")
    finally:
        gpu.close()


def test_two_replicas_on_one_device(box):
    sc, cam, _ = box
    opt = scenes.options(2048, 2048, 16, 16)
    replicas = [binding.Scene(sc, device=0), binding.Scene(sc, device=0)]
    try:
        full = binding.process_job_multi(replicas, cam, opt, base_seed=SEED)
        frame = binding.Frame(replicas, cam, opt, base_seed=SEED)
        try:
            control, progress = _cancel_after(1)
            _, _, info = frame.render(progress=progress, control=control)
            assert info["status"] == binding.PT_ERR_CANCELLED and len(info["stats"]) == 2
            assert info["frame"]["streams_parked"] > 0
            assert_bits_equal(_finish(frame), full, "two replicas stopped and resumed")
        finally:
            frame.close()
    finally:
        for r in replicas:
            r.close()


def test_isolation_between_slices(box):
    sc, cam, gpu = box
    opt = scenes.options(2048, 2048, 16, 16)
    full = gpu.process_job(cam, opt, base_seed=SEED)
    fresh = binding.Scene(sc, device=0)
    try:
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        try:
            control, progress = _cancel_after(1)
            _, _, info = frame.render(progress=progress, control=control)
            assert info["status"] == binding.PT_ERR_CANCELLED and info["frame"]["streams_parked"] > 0
            # the same scene renders something else between two slices of the frame
            small = scenes.options(200, 120, 4, 12)
            assert_bits_equal(gpu.process_job(cam, small, base_seed=5), fresh.process_job(cam, small, base_seed=5), "process_job between slices")
            streams = binding.pixel_streams(np.array([3, 10, 40]), np.array([5, 20, 47]), np.array([11, 22, 33], np.uint64))
            streams["w"][1], streams["h"][1] = 6, 4
            a_img, a_states = gpu.process_item(cam, small, streams)
            b_img, b_states = fresh.process_item(cam, small, streams)
            assert_bits_equal(a_img, b_img, "process_item between slices")
            assert (a_states == b_states).all()
            assert_bits_equal(_finish(frame), full, "frame resumed after other renders on its scene")
        finally:
            frame.close()
        # two frames with different seeds on one scene, their slices interleaved
        opt = scenes.options(512, 512, 32, 32)
        want_a, want_b = fresh.process_job(cam, opt, base_seed=SEED), fresh.process_job(cam, opt, base_seed=SEED + 1)
        a = binding.Frame(gpu, cam, opt, base_seed=SEED)
        b = binding.Frame(gpu, cam, opt, base_seed=SEED + 1)
        try:
            for _ in range(MAX_CALLS):
                if a.done and b.done:
                    break
                for f in (a, b):
                    if not f.done:
                        control, progress = _cancel_after(3)
                        f.render(progress=progress, control=control)
            assert a.done and b.done
            assert_bits_equal(a.image, want_a, "interleaved frame, seed %d" % SEED)
            assert_bits_equal(b.image, want_b, "interleaved frame, seed %d" % (SEED + 1))
        finally:
            a.close()
            b.close()
    finally:
        fresh.close()


def test_progress_increases_across_calls(box):
    _, cam, gpu = box
    opt = scenes.options(1024, 1024, 16, 16)
    frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
    n_tiles = len(frame.tiles)
    reports = []
    try:
        for _ in range(MAX_CALLS):
            control = binding.RenderControl()

            def progress(done, total):
                reports.append((done, total))
                if len(reports) % 5 == 0:
                    control.cancel()
            _, _, info = frame.render(progress=progress, control=control)
            if info["status"] == binding.PT_OK:
                break
        assert frame.done
        done = [d for d, _ in reports]
        assert all(t == n_tiles for _, t in reports)
        assert done == list(range(1, n_tiles + 1)), "progress must count every tile once, strictly increasing across calls"
        assert reports[-1] == (n_tiles, n_tiles)
    finally:
        frame.close()


def test_cpp_frame_render(tmp_path):
    exe = str(tmp_path / "frame_render_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "frame_render_test.cpp")], exe, extra_flags=["-O1"])
    path = [build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]
    r = subprocess.run([exe], env=dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(path)), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[ OK ]") == 5, r.stdout
