"""Resumable view batches on the GPU (pt_frame_create_views, binding.ViewsFrame, PathTrace/view_batch_render.h) and the batched feature pass
and filter behind their denoised form (pt_render_features_views, pt_denoise_views): however a batch was sliced it equals process_views bit
for bit, its preview is the single frame's per view, and every batched stage gives each view what the single-frame call gives it alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from cpupathtrace_amd import binding, build_host, scenes
from tests import denoise_ref, preview_ref, views_ref
from tests.util import assert_bits_equal, env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [11, 2024, 77, 9001, 123456789012, 5, 6, 7]
MAX_CALLS = 60


def _views(cam, n):
    """n cameras around `cam`: pinhole, circular and hexagonal aperture in turn, each from a different place (as tests/test_gpu_views.py)."""
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


def _cancel_after(n_tiles):
    """A control and a progress callback that cancels it once `n_tiles` tiles of the call have been reported."""
    control = binding.RenderControl()
    seen = []

    def progress(done, total):
        seen.append(done)
        if len(seen) == n_tiles:
            control.cancel()
    return control, progress


def _finish(frame):
    img, tile_done, info = frame.render()
    assert info["status"] == binding.PT_OK and tile_done.all() and frame.done
    return img


def _slice_by_budget(frame, budget_ms=50.0):
    """Budgeted slices until the frame is done; the budget doubles after a call that parked nothing (a budget shorter than the launch's
    start-up ends every call before it has resumed anything).  Returns the calls' infos."""
    infos = []
    while not frame.done:
        assert len(infos) < MAX_CALLS, "the frame did not finish in %d slices" % MAX_CALLS
        _, _, info = frame.render(budget_ms=budget_ms)
        infos.append(info)
        if info["streams_abandoned"] == 0:
            budget_ms *= 2.0
    return infos


@pytest.fixture(scope="module")
def box():
    sc, cam = scenes.box_scene()
    gpu = binding.Scene(sc, device=0)
    yield sc, cam, gpu
    gpu.close()


# ---- 1. sliced equals unsliced ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell", "box"])
@pytest.mark.parametrize("spp", [(4, 4), (2, 24)], ids=["fixed", "adaptive"])
def test_sliced_equals_unsliced(name, spp):
    w, h = 203, 157  # tile size 32: clipped edge tiles in both directions
    sc, cam = scenes.cornell_scene(w, h) if name == "cornell" else scenes.box_scene()
    gpu = binding.Scene(sc, device=0)
    try:
        opt = scenes.options(w, h, *spp)
        cams = _views(cam, 3)
        cams[1]["aperture_width"] = cams[1]["aperture_height"] = 0.09
        want = gpu.process_views(cams, opt, base_seeds=SEEDS[:3])
        frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=SEEDS[:3])
        try:
            assert frame.image.shape == (3, h, w, 4)
            calls = 0
            while not frame.done:
                assert calls < MAX_CALLS
                control, progress = _cancel_after(1)
                frame.render(budget_ms=50, progress=progress, control=control)
                calls += 1
            # (a batch this small may finish inside its first slice; test_restore_path_was_used is the one that insists on a stop)
            print("%s %s: %d calls" % (name, spp, calls))
            assert_bits_equal(frame.image, want, "%s %s sliced view frame" % (name, spp))
        finally:
            frame.close()
    finally:
        gpu.close()


# ---- 2. the restore path was really used -----------------------------------------------------------------------------------------------

def test_restore_path_was_used(box):
    _, cam, gpu = box
    opt = scenes.options(256, 256, 1024, 1024)
    cams = _views(cam, 8)
    want = gpu.process_views(cams, opt, base_seeds=SEEDS)
    frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=SEEDS)
    try:
        # Every pixel of this batch is in flight at once and takes 1024 samples, so the slices' progress is the samples the parked pixels
        # carry.  A stopped call costs tens of ms of its own, so a 50 ms slice adds little: the bound on the calls is wide.
        infos, restored, views_parked, budget_ms, carried, max_calls = [], False, 0, 50.0, 0, 300
        while not frame.done:
            assert len(infos) < max_calls, "the frame did not finish in %d slices" % max_calls
            _, _, info = frame.render(budget_ms=budget_ms)
            infos.append(info)
            fi = info["frame"]
            if info["status"] == binding.PT_ERR_CANCELLED and info["streams_finished"] == 0 and fi["samples_carried"] <= carried:
                budget_ms *= 2.0  # (the call added no sample: the budget ran out before its launch had resumed the parked pixels)
            carried = fi["samples_carried"]
            if info["status"] == binding.PT_ERR_CANCELLED and fi["streams_parked"] > 0 and fi["samples_carried"] > 0:
                restored = True
                samples = frame.preview()[1]
                views_parked = max(views_parked, int((samples >= 1).any(axis=(1, 2)).sum()))
            if info["streams_abandoned"] == 0:
                budget_ms *= 2.0
        print("8 x 256^2 x 1024 spp: %d calls; parked per call %s; views with parked pixels %d" %
              (len(infos), [i["streams_abandoned"] for i in infos], views_parked))
        assert restored, "no call stopped with parked streams that carry samples: the restore path was not used"
        assert views_parked >= 2, "parked pixels lay in %d view(s)" % views_parked
        assert len(infos) >= 3, "the frame took %d calls" % len(infos)
        assert_bits_equal(frame.image, want, "view frame sliced by budget")
    finally:
        frame.close()


# ---- 3. adaptive estimator carried -----------------------------------------------------------------------------------------------------

def test_adaptive_estimator_is_carried_over():
    desc, cam = _lit_room(2)
    gpu = binding.Scene(desc, device=0)
    try:
        opt = scenes.options(512, 512, 16, 64)
        cams = _views(cam, 8)  # (2 M pixels: more streams than slots, a stop finds most pixels half-way)
        want = gpu.process_views(cams, opt, base_seeds=SEEDS)
        frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=SEEDS)
        try:
            control, progress = _cancel_after(2)
            _, _, info = frame.render(progress=progress, control=control)
            fi = info["frame"]
            print("adaptive: %s" % fi)
            assert info["status"] == binding.PT_ERR_CANCELLED
            assert fi["streams_parked"] > 0 and fi["parked_with_candidates"] > 0, "no parked stream holds closed candidates"
            assert_bits_equal(_finish(frame), want, "adaptive view frame resumed after a cancel")
        finally:
            frame.close()
    finally:
        gpu.close()


# ---- 4. one view is a Frame ------------------------------------------------------------------------------------------------------------

def test_one_view_is_a_frame(box):
    _, cam, gpu = box
    opt = scenes.options(1024, 768, 8, 24)
    c = _views(cam, 2)[1]
    a = binding.ViewsFrame(gpu, [c], opt, base_seeds=[SEEDS[1]])
    b = binding.Frame(gpu, c, opt, base_seed=SEEDS[1])
    try:
        assert (a.tiles == b.tiles).all()
        ia, ib = a.info(), b.info()
        assert ia == ib
        a.render()
        b.render()
        assert a.image.shape == (1,) + b.image.shape
        assert_bits_equal(a.image[0], b.image, "a view frame of one view")
        ia, ib = a.info(), b.info()
        assert ia == ib, (ia, ib)
        assert_bits_equal(a.image[0], gpu.process_job(c, opt, base_seed=SEEDS[1]), "a view frame of one view against process_job")
    finally:
        a.close()
        b.close()


# ---- 5. every kernel variant -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["lds_window8", "lds_window4", "hbm_tree", "wide_word"])
def test_every_kernel_variant(variant):
    knobs = {}
    if variant == "lds_window8":
        sc, cam = scenes.cornell_scene(256, 256)
        knobs = {"PT_STACK_WINDOW": 8}
    elif variant == "lds_window4":
        sc, cam = scenes.box_scene()
        knobs = {"PT_STACK_WINDOW": 4}
    elif variant == "hbm_tree":
        mesh = scenes.bumpy_sphere_mesh(230, 230, scenes.DRAGON_BOX_TRANSFORM)
        assert len(mesh[0]) >= 100000
        sc, cam = scenes.dragon_box_scene(*mesh)
    else:
        sc, cam = _lit_room(12)
    with env(PT_DEBUG="0", **knobs):
        gpu = binding.Scene(sc, device=0)
        try:
            opt = scenes.options(256, 256, 8, 48)
            cams = _views(cam, 3)
            want = gpu.process_views(cams, opt, base_seeds=SEEDS[:3])
            frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=SEEDS[:3])
            try:
                control, progress = _cancel_after(1)
                _, tile_done, info = frame.render(progress=progress, control=control)
                print("%s: %s" % (variant, info["frame"]))
                assert info["status"] == binding.PT_ERR_CANCELLED and not tile_done.all()
                assert info["frame"]["streams_parked"] > 0, "%s: the stop parked nothing" % variant
                assert_bits_equal(_finish(frame), want, "%s: view frame stopped and resumed" % variant)
            finally:
                frame.close()
        finally:
            gpu.close()


# ---- 6. two replicas -------------------------------------------------------------------------------------------------------------------

def _owners(tiles, n_scenes):
    """The replica of every tile, as the library deals them (along the diagonals of a grid whose rows hold a multiple of n_scenes tiles)."""
    per_row = int((tiles["y"] == tiles["y"][0]).argmin()) or len(tiles)
    k = np.arange(len(tiles))
    diagonal = len(tiles) % per_row == 0 and per_row % n_scenes == 0
    return ((k % per_row + k // per_row) if diagonal else k) % n_scenes


def test_two_replicas_on_one_device(box):
    sc, cam, gpu = box
    opt = scenes.options(512, 512, 256, 256)
    cams = _views(cam, 8)
    want = gpu.process_views(cams, opt, base_seeds=SEEDS)
    replicas = [binding.Scene(sc, device=0), binding.Scene(sc, device=0)]
    try:
        frame = binding.ViewsFrame(replicas, cams, opt, base_seeds=SEEDS)
        try:
            owner = np.zeros((8 * 512, 512), np.int32)
            for t, o in zip(frame.tiles, _owners(frame.tiles, 2)):
                owner[t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]] = o
            # budgeted slices until stops have parked pixels of both replicas -- not necessarily the same stop: the two persistent
            # launches share one device, and one of them may fill it while the other waits
            seen, budget_ms = [False, False], 50.0
            for _ in range(MAX_CALLS):
                _, _, info = frame.render(budget_ms=budget_ms)
                assert len(info["stats"]) == 2
                if info["status"] == binding.PT_OK:
                    break
                parked = frame.preview()[1].reshape(-1, 512) >= 1
                print("two replicas: parked %d and %d" % (parked[owner == 0].sum(), parked[owner == 1].sum()))
                seen = [seen[i] or bool(parked[owner == i].any()) for i in range(2)]
                if all(seen):
                    break
                if info["streams_abandoned"] == 0:
                    budget_ms *= 2.0
            assert all(seen), "replicas that parked pixels in some stop: %s" % seen
            assert_bits_equal(_finish(frame), want, "two replicas stopped and resumed against one replica's process_views")
        finally:
            frame.close()
    finally:
        for r in replicas:
            r.close()


# ---- 7. isolation ----------------------------------------------------------------------------------------------------------------------

def test_isolation_between_slices(box):
    sc, cam, gpu = box
    opt = scenes.options(512, 512, 16, 16)
    cams = _views(cam, 8)
    want = gpu.process_views(cams, opt, base_seeds=SEEDS)
    fresh = binding.Scene(sc, device=0)
    frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=SEEDS)
    try:
        control, progress = _cancel_after(1)
        _, _, info = frame.render(progress=progress, control=control)
        assert info["status"] == binding.PT_ERR_CANCELLED and info["frame"]["streams_parked"] > 0
        # another batch with other cameras, more of them, and a plain job on the same scene between two slices
        small = scenes.options(64, 48, 4, 12)
        others = [dict(c, origin=(c["origin"][0] - 0.3, c["origin"][1] + 0.2, c["origin"][2])) for c in _views(cam, 11)]
        seeds = list(range(100, 111))
        assert_bits_equal(gpu.process_views(others, small, base_seeds=seeds), fresh.process_views(others, small, base_seeds=seeds), "process_views between slices")
        assert_bits_equal(gpu.process_job(cam, small, base_seed=5), fresh.process_job(cam, small, base_seed=5), "process_job between slices")
        gpu.render_features_views(others, small)
        assert_bits_equal(_finish(frame), want, "view frame resumed after another batch on its scene")
    finally:
        frame.close()
        fresh.close()


# ---- 8. progress -----------------------------------------------------------------------------------------------------------------------

def test_progress_increases_across_calls(box):
    _, cam, gpu = box
    opt = scenes.options(256, 256, 16, 16)
    cams = _views(cam, 5)
    frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=SEEDS[:5])
    n_tiles = 5 * len(binding.job_tiles(256, 256))
    assert len(frame.tiles) == n_tiles
    reports = []
    try:
        for _ in range(MAX_CALLS):
            control = binding.RenderControl()

            def progress(done, total):
                reports.append((done, total))
                if len(reports) % 37 == 0:
                    control.cancel()
            _, tile_done, info = frame.render(progress=progress, control=control)
            assert len(tile_done) == n_tiles
            if info["status"] == binding.PT_OK:
                break
        assert frame.done and tile_done.all()
        assert all(t == n_tiles for _, t in reports)
        assert [d for d, _ in reports] == list(range(1, n_tiles + 1)), "progress must count every tile once, strictly increasing across calls"
        assert frame.info()["tiles_total"] == n_tiles and frame.info()["tiles_done"] == n_tiles
    finally:
        frame.close()


# ---- 9. and 11. the preview of a stopped view frame ------------------------------------------------------------------------------------

# 1.5 M pixels of 1024 samples each: one MI355X keeps 1,048,576 streams in flight, exactly four of these views, and a first
# slice too short for any pixel to finish takes no further stream -- the last two views are still holes after it
STOPPED_OPT = scenes.options(512, 512, 1024, 1024)
STOPPED_VIEWS = 6


@pytest.fixture(scope="module")
def stopped(box):
    sc, cam, gpu = box
    cams = _views(cam, STOPPED_VIEWS)
    seeds = SEEDS[:STOPPED_VIEWS]
    frame = binding.ViewsFrame(gpu, cams, STOPPED_OPT, base_seeds=seeds)
    budget_ms = 20.0
    for _ in range(MAX_CALLS):
        _, _, info = frame.render(budget_ms=budget_ms)
        assert info["status"] == binding.PT_ERR_CANCELLED, "the batch finished inside a %.0f ms slice" % budget_ms
        if info["frame"]["streams_parked"] > 0:
            break
        budget_ms *= 2.0
    raw, samples = frame.preview()
    print("stopped view frame: %s; pixels with samples per view %s" % (info["frame"], [(int((s != 0).sum())) for s in samples]))
    yield sc, cams, seeds, gpu, frame, info["frame"], raw, samples
    frame.close()


def test_raw_preview(stopped):
    sc, cams, seeds, gpu, frame, fi, raw, samples = stopped
    finished, parked, holes = samples == -1, samples >= 1, samples == 0
    assert raw.shape == frame.image.shape and samples.shape == frame.image.shape[:3]
    assert (samples >= -1).all()
    assert int(finished.sum()) == fi["streams_finished"] and int(parked.sum()) == fi["streams_parked"] and int(holes.sum()) == fi["streams_untouched"]
    assert fi["streams_parked"] > 0 and fi["streams_untouched"] > 0
    assert int(samples[parked].astype(np.int64).sum()) == fi["samples_carried"]
    assert_bits_equal(raw[finished], frame.image[finished], "finished pixels")
    assert (raw[holes] == 0).all(), "holes"
    # a parked pixel has taken samples; it shows their mean, alpha 1 -- or, by the preview's contract (pt_hip.h), (0, 0, 0, 0) while none of
    # its samples has been collected (the oracle comparison below includes such pixels)
    assert (samples[parked] >= 1).all()
    alpha = raw[parked][:, 3]
    empty = alpha != 1.0
    assert (raw[parked][empty] == 0).all(), "a parked pixel's alpha is neither 1 nor that of a pixel without a collected sample"
    print("parked pixels without a collected sample: %d of %d" % (int(empty.sum()), len(alpha)))
    assert empty.sum() * 20 <= len(alpha)
    views_with_parked = [v for v in range(len(cams)) if parked[v].any()]
    assert len(views_with_parked) >= 2, "parked pixels lie in views %s only" % views_with_parked
    chk = oracle.Checker("oracle")
    h = chk.scene_create(sc)
    try:
        for v in (views_with_parked[0], views_with_parked[-1]):
            ys, xs = np.nonzero(parked[v])
            pick = np.random.default_rng(len(xs) + v).choice(len(xs), min(96, len(xs)), replace=False)
            none_collected = np.nonzero(raw[v][ys, xs][:, 3] != 1.0)[0][:16]
            pick = np.union1d(pick, none_collected)
            xs, ys = xs[pick], ys[pick]
            want = preview_ref.raw_preview(h, cams[v], STOPPED_OPT, seeds[v], xs, ys, samples[v][ys, xs], binding.pixel_seed, binding.seed_to_state)
            assert_bits_equal(raw[v][ys, xs], want, "view %d: parked pixels against the oracle's running mean" % v)
    finally:
        h.close()


def test_masked_view_filter(stopped):
    sc, cams, seeds, gpu, frame, fi, raw, samples = stopped
    got, samples2 = frame.preview(denoise=True)
    assert (samples2 == samples).all()
    feats = gpu.render_features_views(cams, STOPPED_OPT)
    want = views_ref.preview_denoise_views(raw, feats, samples, **denoise_ref.DEFAULTS)
    print("largest difference %.3g" % np.nanmax(np.abs(got.astype(np.float64) - want)))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)
    empty = [v for v in range(len(cams)) if (samples[v] == 0).all()]
    assert empty, "no view is entirely holes: pixels with samples per view %s" % [int((s != 0).sum()) for s in samples]
    for v in empty:
        assert (got[v] == 0).all(), "view %d is all holes and was filled from another view" % v
    # ... and the view above the first empty one has pixels with samples within the filter's reach of the border (2 * 16 rows in 5 passes)
    assert empty[0] > 0 and (samples[empty[0] - 1][-32:] != 0).any(), "no pixel with samples lies within reach of an empty view"


def test_masked_view_filter_fills_holes_inside_a_view(box):
    """A stop late enough for freed slots to have started on the next view: that view has pixels with samples and holes side by side."""
    _, cam, gpu = box
    opt = scenes.options(512, 512, 32, 32)
    cams = _views(cam, 6)
    frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=SEEDS[:6])
    try:
        control, progress = _cancel_after(1)
        _, _, info = frame.render(progress=progress, control=control)
        assert info["status"] == binding.PT_ERR_CANCELLED
        raw, samples = frame.preview()
        got, _ = frame.preview(denoise=True)
        print("pixels with samples per view %s" % [int((s != 0).sum()) for s in samples])
        mixed = [v for v in range(6) if (samples[v] == 0).any() and (samples[v] != 0).any()]
        assert mixed, "no view has both holes and pixels with samples"
        want = views_ref.preview_denoise_views(raw, gpu.render_features_views(cams, opt), samples, **denoise_ref.DEFAULTS)
        print("largest difference %.3g" % np.nanmax(np.abs(got.astype(np.float64) - want)))
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)
        holes = samples == 0
        filled = got[holes][:, 3] == 1.0
        assert filled.any() and (got[holes][~filled] == 0).all()
    finally:
        frame.close()


def test_preview_changes_nothing(stopped):
    """(after the two tests above: the frame has been previewed raw and denoised)"""
    sc, cams, seeds, gpu, frame, fi, raw, samples = stopped
    assert_bits_equal(_finish(frame), gpu.process_views(cams, STOPPED_OPT, base_seeds=seeds), "a view frame finished after its previews")
    rgba, samples = frame.preview()
    assert (samples == -1).all()
    assert_bits_equal(rgba, frame.image, "the preview of a complete view frame")


def test_complete_frame_denoised_preview(box):
    _, cam, gpu = box
    opt = scenes.options(96, 72, 16, 16)
    cams = _views(cam, 3)
    frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=SEEDS[:3])
    try:
        frame.render()
        clean, samples = frame.preview(denoise=True)
        assert (samples == -1).all()
        for v in range(3):
            assert_bits_equal(clean[v], gpu.process_job(cams[v], opt, base_seed=SEEDS[v], allow_bias=True), "denoised preview, view %d" % v)
    finally:
        frame.close()


def test_fresh_frame_is_all_holes(box):
    _, cam, gpu = box
    frame = binding.ViewsFrame(gpu, _views(cam, 3), scenes.options(80, 50, 8, 8))
    try:
        for denoise in (None, True):
            rgba, samples = frame.preview(denoise=denoise)
            assert rgba.shape == (3, 50, 80, 4) and samples.shape == (3, 50, 80)
            assert (rgba == 0).all() and (samples == 0).all()
        assert frame.info()["launches"] == 0
    finally:
        frame.close()


# ---- 10. batched features and filter ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box", "mesh"])
def test_batched_features_and_filter(box, name):
    if name == "box":
        _, cam, gpu = box
    else:
        sc, cam = scenes.dragon_box_scene(*scenes.bumpy_sphere_mesh(120, 120, scenes.DRAGON_BOX_TRANSFORM))
        gpu = binding.Scene(sc, device=0)
    try:
        opt = scenes.options(96, 72, 4, 4)
        cams = _views(cam, 5)
        images = gpu.process_views(cams, opt, base_seeds=SEEDS[:5])
        feats = gpu.render_features_views(cams, opt)
        assert feats.shape == (5, 72, 96, 3, 4)
        for v in range(5):
            assert_bits_equal(feats[v], gpu.render_features(cams[v], opt), "%s features, view %d" % (name, v))
        assert not (feats[0] == feats[1]).all()
        for params in (None, {"iterations": 0}, {"iterations": 10}):
            got = binding.denoise_views(images, feats, params=params)
            for v in range(5):
                assert_bits_equal(got[v], binding.denoise(images[v], feats[v], params=params), "%s filter %s, view %d" % (name, params, v))
        # one view is the single-frame call
        assert_bits_equal(gpu.render_features_views(cams[3:4], opt)[0], gpu.render_features(cams[3], opt), "one view's features")
        assert_bits_equal(binding.denoise_views(images[3:4], feats[3:4])[0], binding.denoise(images[3], feats[3]), "one view's filter")
    finally:
        if name != "box":
            gpu.close()


DEVICE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding, scenes
V, W, H = 5, 96, 72
d_feat = torch.full((V, H, W, 3, 4), -7.0, dtype=torch.float32, device="cuda:0")
sc, cam = scenes.box_scene()
gpu = binding.Scene(sc, device=0)
opt = scenes.options(W, H, 4, 4)
cams = [dict(cam, origin=(cam["origin"][0] + 0.07 * v, cam["origin"][1], cam["origin"][2] - 0.02 * v)) for v in range(V)]
stream = torch.cuda.current_stream(0).cuda_stream
feat = gpu.render_features_views(cams, opt)
gpu.render_features_views_device(cams, opt, d_feat.data_ptr(), stream)
torch.cuda.synchronize()
checks = {"render_features_views_device": (d_feat.cpu().numpy(), feat)}
noisy = gpu.process_views(cams, opt, base_seeds=5)
once = binding.denoise_views(noisy, feat)
d_img = torch.from_numpy(noisy).to("cuda:0")
d_out = torch.empty_like(d_img)
binding.denoise_views_device(d_img.data_ptr(), d_feat.data_ptr(), W, H, V, d_out.data_ptr(), stream)
checks["denoise_views_device"] = (d_out.cpu().numpy(), once)
binding.denoise_views_device(d_img.data_ptr(), d_feat.data_ptr(), W, H, V, d_img.data_ptr(), stream)
checks["denoise_views_device in place"] = (d_img.cpu().numpy(), once)
ok = True
for what, (got, want) in checks.items():
    same = bool((got.view(np.uint32) == want.view(np.uint32)).all())
    print("%s: %s" % (what, "bit-identical" if same else "DIFFERENT"))
    ok = ok and same
sys.exit(0 if ok else 1)
"""


def test_device_memory_forms():
    """The _device forms on torch tensors equal the host forms bit for bit (in a fresh interpreter in which torch opens the device first, as
    tests/test_gpu_denoise.py does)."""
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("bit-identical") == 3, r.stdout


def test_batched_filter_does_not_cross_view_borders(box):
    """Two stacks that differ in one view only: every other view's result keeps its bits."""
    _, cam, gpu = box
    opt = scenes.options(96, 72, 4, 4)
    cams = _views(cam, 3)
    images = gpu.process_views(cams, opt, base_seeds=SEEDS[:3])
    feats = gpu.render_features_views(cams, opt)
    a = binding.denoise_views(images, feats, params={"iterations": 10})
    images2, feats2 = images.copy(), feats.copy()
    images2[1, :, :, :3] *= 7.0
    feats2[1] = feats[2]
    b = binding.denoise_views(images2, feats2, params={"iterations": 10})
    assert_bits_equal(b[0], a[0], "view 0 beside a changed view 1")
    assert_bits_equal(b[2], a[2], "view 2 beside a changed view 1")
    assert not (b[1] == a[1]).all()


# ---- 12. the C++ program ---------------------------------------------------------------------------------------------------------------

def test_cpp_view_batch_render(tmp_path):
    exe = str(tmp_path / "view_batch_render_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "view_batch_render_test.cpp")], exe, extra_flags=["-O1"])
    path = [build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]
    r = subprocess.run([exe], env=dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(path)), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[ OK ]") == 3, r.stdout
