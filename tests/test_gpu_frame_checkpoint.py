"""Checkpoints of a frame on the GPU (pt_frame_checkpoint_save / _load, binding.Frame.checkpoint / save / restore; include/pt_checkpoint.h,
DESIGN.md 4.18): a frame saved between two render calls and loaded onto a fresh scene -- on the same or another number of replicas --
reports, previews and rates as the original does, saves the same bytes again, and finishes bit-identically to one uninterrupted
process_job.  The scenes are those of tests/test_gpu_frame_resume.py; the stops are progressive passes wherever a test needs the same state
twice."""
import os
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build_host, scenes
from tests import checkpoint_ref as ref
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2718
QUANTUM = 8
MAX_CALLS = 40
PT_ERR_INVALID = 1


def _lit_room(n_point_lights):
    """The lit room of tests/test_gpu_frame_resume.py."""
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
    control = binding.RenderControl()
    seen = []

    def progress(done, total):
        seen.append(done)
        if len(seen) == n_tiles:
            control.cancel()
    return control, progress


def _finish(frame):
    """Render the rest of a frame, whatever mode it is in; returns the image."""
    for _ in range(MAX_CALLS * 4):
        img, tile_done, info = frame.render()
        if info["status"] == binding.PT_OK:
            assert tile_done.all() and frame.done
            return img
    raise AssertionError("the frame did not finish")


def _pass(frame):
    frame.set_progressive(QUANTUM, 1)
    _, _, info = frame.render()
    return info


def _state(frame, denoise=None):
    """What a frame reports and shows between two calls."""
    info = {k: v for k, v in frame.info().items() if k != "park_bytes"}
    rgba, samples = frame.preview(denoise)
    return dict(info=info, progress=frame.progress(), rgba=rgba, samples=samples, error=frame.error_map(), variance=frame.variance())


def _assert_same_state(a, b, what):
    assert a["info"] == b["info"], (what, a["info"], b["info"])
    assert a["progress"] == b["progress"], (what, a["progress"], b["progress"])
    assert (a["samples"] == b["samples"]).all(), what
    for key in ("rgba", "error", "variance"):
        assert_bits_equal(b[key], a[key], "%s: %s" % (what, key))


@pytest.fixture(scope="module")
def room():
    """The lit room on the GPU, and -- computed once, never changed -- its uninterrupted 96 x 64 adaptive frame."""
    desc, cam = _lit_room(2)
    gpu = binding.Scene(desc, device=0)
    opt = scenes.options(96, 64, 16, 64)
    full = gpu.process_job(cam, opt, base_seed=SEED)
    full.setflags(write=False)
    yield dict(desc=desc, cam=cam, gpu=gpu, opt=opt, full=full)
    gpu.close()


def _save_load_finish(room, frame, what, n_replicas=1, denoise=None):
    """Saves `frame`, loads the blob into a fresh Frame on fresh Scenes, holds both against each other, finishes both."""
    blob = frame.checkpoint()
    assert (frame.checkpoint() == blob).all(), "%s: a second save gives other bytes" % what
    fresh = [binding.Scene(room["desc"], device=0) for _ in range(n_replicas)]
    try:
        loaded = binding.Frame.restore(fresh, blob)
        try:
            assert type(loaded) is binding.Frame
            _assert_same_state(_state(frame, denoise), _state(loaded, denoise), what)
            again = loaded.checkpoint()
            assert again.tobytes() == blob.tobytes(), "%s: the loaded frame saves other bytes" % what
            assert_bits_equal(_finish(loaded), room["full"], what + ": the loaded frame, finished")
        finally:
            loaded.close()
        assert_bits_equal(_finish(frame), room["full"], what + ": the saved frame, finished")
    finally:
        for s in fresh:
            s.close()
    return blob


# ---- 5. records everywhere --------------------------------------------------------------------------------------------------------------

def test_after_one_pass_every_stream_has_a_record(room):
    frame = binding.Frame(room["gpu"], room["cam"], room["opt"], base_seed=SEED)
    try:
        info = _pass(frame)
        assert info["status"] == binding.PT_ERR_CANCELLED
        fi = frame.info()
        assert fi["streams_parked"] == 96 * 64 and fi["streams_finished"] == 0 and fi["parked_with_candidates"] == 0
        blob = frame.checkpoint()
        got = binding.checkpoint_inspect(blob)
        assert (got["streams_with_record"], got["streams_finished"], got["streams_untouched"], got["streams_with_candidates"]) == (96 * 64, 0, 0, 0)
        # a record without candidates is 144 of the 528 bytes of its park record: 27 %
        assert got["bytes_records"] == 144 * 96 * 64 and round(100.0 * got["bytes_records"] / (528 * 96 * 64)) == 27
        assert got["quantum"] == QUANTUM and got["target"] == QUANTUM and got["passes_completed"] == 1 and got["pass_in_progress"] == 0 and got["launches"] == 1
        # the blob reads back through the independent reader, and its records are the pixels the preview shows
        parts = ref.read(blob.tobytes())
        assert ref.inspect(blob.tobytes())["streams_with_record"] == 96 * 64 and len(parts["records"]) == 96 * 64
        assert all(int(r[ref.PIXEL_SAMPLE_WORD]) == QUANTUM and int(r[ref.EST_PAD_WORD]) == 0 and int(r[3]) == 0 for r in parts["records"][::97])
        _save_load_finish(room, frame, "after one pass")
    finally:
        frame.close()


def test_candidates_and_finished_pixels_together(room):
    frame = binding.Frame(room["gpu"], room["cam"], room["opt"], base_seed=SEED)
    try:
        for passes in range(1, MAX_CALLS + 1):
            info = _pass(frame)
            fi = frame.info()
            if fi["parked_with_candidates"] > 0 and fi["streams_finished"] > 0:
                break
            assert info["status"] == binding.PT_ERR_CANCELLED, "the frame finished before it held candidates and finished pixels together"
        else:
            raise AssertionError("no pass left records with candidates next to finished pixels")
        print("after %d passes: %s" % (passes, fi))
        assert fi["streams_parked"] > 0
        blob = _save_load_finish(room, frame, "after %d passes" % passes)
        got = binding.checkpoint_inspect(blob)
        assert got["streams_with_candidates"] == fi["parked_with_candidates"] and got["streams_finished"] == fi["streams_finished"]
        parts = ref.read(blob.tobytes())
        k = (parts["map"] >> 2)[(parts["map"] & 3) == ref.RECORD]
        assert got["bytes_records"] == int((144 + 48 * k.astype(np.int64)).sum()) < 528 * len(k)
        for r, kk in list(zip(parts["records"], k.tolist()))[::53]:
            assert int(r[ref.N_CANDIDATES_WORD]) == kk and int(r[ref.EST_PAD_WORD]) == 0
            assert all((r[36 + 12 * c + 9:36 + 12 * c + 12] == 0).all() for c in range(kk))
    finally:
        frame.close()


# ---- 6. a plain frame with all three classes ---------------------------------------------------------------------------------------------

def test_plain_frame_with_finished_parked_and_untouched_streams():
    desc, cam = _lit_room(12)
    gpu, fresh = binding.Scene(desc, device=0), binding.Scene(desc, device=0)
    try:
        opt = scenes.options(2048, 2048, 8, 8)
        full = gpu.process_job(cam, opt, base_seed=SEED)
        frame = binding.Frame(gpu, cam, opt, base_seed=SEED)
        try:
            control, progress = _cancel_after(1)
            _, tile_done, info = frame.render(progress=progress, control=control)
            assert info["status"] == binding.PT_ERR_CANCELLED and not tile_done.all()
            blob = frame.checkpoint()
            got = binding.checkpoint_inspect(blob)
            print("plain frame: %s" % {k: got[k] for k in ("streams_finished", "streams_with_record", "streams_untouched", "total_bytes")})
            assert got["streams_finished"] > 0 and got["streams_with_record"] > 0 and got["streams_untouched"] > 0
            fi = frame.info()
            assert (got["streams_finished"], got["streams_with_record"], got["streams_untouched"]) == (fi["streams_finished"], fi["streams_parked"], fi["streams_untouched"])
            loaded = binding.Frame.restore(fresh, blob)
            try:
                assert {k: v for k, v in loaded.info().items() if k != "park_bytes"} == {k: v for k, v in fi.items() if k != "park_bytes"}
                assert_bits_equal(loaded.image, np.where((loaded.preview()[1] == -1)[..., None], frame.image, 0), "the finished pixels of the loaded image")
                assert (loaded.checkpoint() == blob).all()
                assert_bits_equal(_finish(loaded), full, "plain frame, loaded and finished")
            finally:
                loaded.close()
            assert_bits_equal(_finish(frame), full, "plain frame, saved and finished")
        finally:
            frame.close()
    finally:
        gpu.close()
        fresh.close()


# ---- 7. the replica count is free --------------------------------------------------------------------------------------------------------

def test_replica_count_is_free(room):
    """One pass leaves the same state whoever renders it, but for the frame's count of launches (one per replica and pass): the blobs of a
    one-replica and a two-replica frame differ in that header field and the checksum only, and a blob loaded onto the other layout saves
    the same bytes again."""
    pair = [binding.Scene(room["desc"], device=0), binding.Scene(room["desc"], device=0)]
    one = binding.Frame(room["gpu"], room["cam"], room["opt"], base_seed=SEED)
    two = binding.Frame(pair, room["cam"], room["opt"], base_seed=SEED)
    try:
        _pass(one), _pass(one), _pass(two), _pass(two)
        blob_one, blob_two = one.checkpoint(), two.checkpoint()
        a, b = np.frombuffer(blob_one[:352].tobytes(), ref.HEADER).copy(), np.frombuffer(blob_two[:352].tobytes(), ref.HEADER).copy()
        assert (int(a["launches"][0]), int(b["launches"][0])) == (2, 4)
        b["launches"] = a["launches"]
        assert a.tobytes() == b.tobytes() and blob_one[352:-8].tobytes() == blob_two[352:-8].tobytes()
        for blob, targets, what in ((blob_one, pair, "saved from one replica, loaded onto two"), (blob_two, [room["gpu"]], "saved from two replicas, loaded onto one")):
            # (the scenes still carry their first frame: a scene may hold several)
            loaded = binding.Frame.restore(targets, blob)
            try:
                assert loaded.checkpoint().tobytes() == blob.tobytes(), what
                _assert_same_state(_state(one if blob is blob_one else two), _state(loaded), what)
                assert_bits_equal(_finish(loaded), room["full"], what)
            finally:
                loaded.close()
        assert_bits_equal(_finish(one), room["full"], "one replica")
        assert_bits_equal(_finish(two), room["full"], "two replicas")
    finally:
        one.close()
        two.close()
        for s in pair:
            s.close()


# ---- the kernels' scans at their edges ------------------------------------------------------------------------------------------------------

def _tiles_of(n, width=64):
    """Rectangles of unequal sizes stacked in an image `width` wide, n pixels in all (as tests/test_checkpoint_cpu.py lays them out)."""
    shapes = [(7, 3), (64, 2), (5, 5), (1, 1), (13, 1), (32, 4), (3, 9)]
    tiles, y, left, i = [], 0, n, 0
    while left > 0:
        w, h = shapes[i % len(shapes)]
        i += 1
        if w * h > left:
            w, h = min(left, width), 1
        tiles.append((0 if i % 2 else width - w, y, w, h))
        y += h
        left -= w * h
    return np.array([tuple(t) for t in tiles], binding.TILE_DTYPE), y


@pytest.fixture(scope="module")
def pair(room):
    scenes_ = [binding.Scene(room["desc"], device=0), binding.Scene(room["desc"], device=0)]
    yield scenes_
    for s in scenes_:
        s.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_stream_counts_at_the_scan_edges(room, pair, n):
    """Frames of 1 .. 2049 streams over unequal tiles (lane, wavefront and scan-workgroup edges; with one tile the second replica has
    none): saved after one pass (records only) and after three (finished pixels next to records with candidates), loaded onto two
    replicas and saved again."""
    tiles, rows = _tiles_of(n)
    opt = scenes.options(64, rows, 16, 64)
    full = room["gpu"].process_job(room["cam"], opt, base_seed=SEED, tiles=tiles)
    frame = binding.Frame(room["gpu"], room["cam"], opt, base_seed=SEED, tiles=tiles)
    try:
        for passes in (1, 2):
            for _ in range(passes):
                _pass(frame)
            blob = frame.checkpoint()
            got = binding.checkpoint_inspect(blob)
            fi = frame.info()
            assert got["n_streams"] == n and (got["streams_finished"], got["streams_with_record"]) == (fi["streams_finished"], fi["streams_parked"])
            parts = ref.read(blob.tobytes())
            samples = frame.preview()[1]
            ys, xs = ref.stream_pixels(np.array([[t["x"], t["y"], t["w"], t["h"]] for t in tiles]))
            assert ((parts["map"] & 3 == ref.FINISHED) == (samples[ys, xs] == -1)).all()
            assert_bits_equal(parts["pixels"], frame.image[ys, xs][parts["map"] & 3 == ref.FINISHED], "the finished pixels of the blob")
            assert [int(r[ref.PIXEL_SAMPLE_WORD]) for r in parts["records"]] == samples[ys, xs][parts["map"] & 3 == ref.RECORD].tolist()
            loaded = binding.Frame.restore(pair, blob)
            try:
                _assert_same_state(_state(frame), _state(loaded), "%d streams after %d passes" % (n, passes))
                assert loaded.checkpoint().tobytes() == blob.tobytes()
                if passes == 2:
                    assert_bits_equal(_finish(loaded), full, "%d streams, loaded onto two replicas and finished" % n)
            finally:
                loaded.close()
        assert_bits_equal(_finish(frame), full, "%d streams, saved and finished" % n)
    finally:
        frame.close()


# ---- 8. views, a noise target, followed features, the two ends of a frame's life ---------------------------------------------------------

def test_view_frame(room):
    cams = []
    for v in range(3):
        c = dict(room["cam"])
        c["origin"] = (0.1 * v, 0.05 * v, -3.0)
        cams.append(c)
    opt = scenes.options(64, 48, 16, 32)
    gpu, fresh = room["gpu"], binding.Scene(room["desc"], device=0)
    try:
        full = gpu.process_views(cams, opt, base_seeds=[SEED, SEED + 1, SEED + 2])
        full = full[0] if isinstance(full, tuple) else full
        frame = binding.ViewsFrame(gpu, cams, opt, base_seeds=[SEED, SEED + 1, SEED + 2])
        try:
            _pass(frame), _pass(frame)
            blob = frame.checkpoint()
            got = binding.checkpoint_inspect(blob)
            assert got["n_views"] == 3 and got["n_streams"] == 3 * 64 * 48 and got["bytes_tables"] == 208 + 24
            loaded = binding.Frame.restore(fresh, blob)
            try:
                assert type(loaded) is binding.ViewsFrame and loaded.image.shape == (3, 48, 64, 4) and (loaded.tiles == frame.tiles).all()
                _assert_same_state(_state(frame), _state(loaded), "view frame")
                assert loaded.checkpoint().tobytes() == blob.tobytes()
                assert_bits_equal(_finish(loaded), full, "view frame, loaded and finished")
            finally:
                loaded.close()
            assert_bits_equal(_finish(frame), full, "view frame, saved and finished")
        finally:
            frame.close()
    finally:
        fresh.close()


def test_noise_target_holds_the_same_streams(room):
    fresh = binding.Scene(room["desc"], device=0)
    frame = binding.Frame(room["gpu"], room["cam"], room["opt"], base_seed=SEED)
    try:
        _pass(frame), _pass(frame)
        error = frame.error_map()
        rated = error[np.isfinite(error) & (error >= 0)]
        assert len(rated) >= 128
        target = float(np.median(rated))
        frame.set_noise_target(target, 1e-5, 1.0)
        info = _pass(frame)
        assert info["status"] == binding.PT_ERR_CANCELLED
        held = frame.noise()["streams_held"]
        assert held > 0
        blob = frame.checkpoint()
        got = binding.checkpoint_inspect(blob)
        assert np.float32(got["noise_target"]) == np.float32(target) and got["noise_fraction"] == 1.0
        loaded = binding.Frame.restore(fresh, blob)
        try:
            assert loaded.noise()["streams_held"] == held
            assert {k: v for k, v in loaded.noise().items() if k != "histogram"} == {k: v for k, v in frame.noise().items() if k != "histogram"}
            _assert_same_state(_state(frame), _state(loaded), "noise target")
            # one more pass leaves the held streams alone in both
            _pass(frame), _pass(loaded)
            _assert_same_state(_state(frame), _state(loaded), "noise target, one pass later")
            assert loaded.checkpoint().tobytes() == frame.checkpoint().tobytes()
            for f in (frame, loaded):
                f.set_noise_target(0.0)
                f.set_progressive(QUANTUM, 0)
            assert_bits_equal(_finish(loaded), room["full"], "noise target cleared, loaded frame finished")
        finally:
            loaded.close()
        assert_bits_equal(_finish(frame), room["full"], "noise target cleared, saved frame finished")
    finally:
        frame.close()
        fresh.close()


def test_followed_features_are_restored(room):
    frame = binding.Frame(room["gpu"], room["cam"], room["opt"], base_seed=SEED)
    try:
        frame.set_feature_params({"max_bounces": 6})
        _pass(frame), _pass(frame)
        got = binding.checkpoint_inspect(frame.checkpoint())
        assert got["follow_features"] == 1
        _save_load_finish(room, frame, "followed features", denoise=True)
    finally:
        frame.close()


def test_saved_before_the_first_launch_and_when_complete(room):
    frame = binding.Frame(room["gpu"], room["cam"], room["opt"], base_seed=SEED)
    try:
        blob = frame.checkpoint()
        got = binding.checkpoint_inspect(blob)
        assert got["streams_untouched"] == 96 * 64 and got["bytes_pixels"] == 0 and got["bytes_records"] == 0 and got["launches"] == 0
        assert blob.tobytes() == ref.write(dict(ref.read(blob.tobytes()), options=tuple(got["options"].values()), n_views=1, cls=np.full(96 * 64, ref.UNTOUCHED, np.uint8),
                                                records=np.zeros((96 * 64, ref.RECORD_WORDS), np.uint32), image=frame.image, launches=0, samples_lost=0,
                                                fingerprint=(np.array([got["fingerprint"][k] for k in ("triangles", "spheres", "materials", "point_lights", "emitters",
                                                                                                        "tree_nodes")], np.uint64), got["fingerprint"]["root_box"])))
        _save_load_finish(room, frame, "before the first launch", n_replicas=2)
        assert frame.done
        blob = frame.checkpoint()
        got = binding.checkpoint_inspect(blob)
        assert got["streams_finished"] == 96 * 64 and got["bytes_pixels"] == 16 * 96 * 64 and got["bytes_records"] == 0
        fresh = binding.Scene(room["desc"], device=0)
        try:
            loaded = binding.Frame.restore(fresh, blob)
            try:
                assert loaded.done
                assert_bits_equal(loaded.image, room["full"], "the image of a complete frame, loaded")
                launches = loaded.info()["launches"]
                img, tile_done, info = loaded.render()
                assert info["status"] == binding.PT_OK and tile_done.all() and loaded.info()["launches"] == launches
                assert loaded.checkpoint().tobytes() == blob.tobytes()
            finally:
                loaded.close()
        finally:
            fresh.close()
    finally:
        frame.close()


def test_save_to_a_file_and_restore_from_it(room, tmp_path):
    frame = binding.Frame(room["gpu"], room["cam"], room["opt"], base_seed=SEED)
    fresh = binding.Scene(room["desc"], device=0)
    try:
        _pass(frame)
        path = tmp_path / "frame.ckpt"
        frame.save(path)
        assert sorted(p.name for p in tmp_path.iterdir()) == ["frame.ckpt"]
        assert path.read_bytes() == frame.checkpoint().tobytes() and binding.checkpoint_inspect(str(path))["streams_with_record"] == 96 * 64
        loaded = binding.Frame.restore(fresh, path)
        try:
            assert_bits_equal(_finish(loaded), room["full"], "restored from a file")
        finally:
            loaded.close()
    finally:
        frame.close()
        fresh.close()


# ---- 9. refusals on the device path --------------------------------------------------------------------------------------------------------

def _mesh_room(extra_sphere):
    """A box with a lamp and one instance of a small mesh (a scene that can be posed); extra_sphere: and one more sphere."""
    sb = scenes.SceneBuilder()
    sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)))
    sb.triangles(scenes.make_plane((-0.25, 0.99, -0.25), (0.25, 0.99, 0.25)), sb.material((1, 1, 1, 1), 1.0, (1, 1, 1, 1)))
    vertices, faces = scenes.bumpy_sphere_vertices(12, 8)
    sb.mesh(vertices, faces, MESH_MATRIX, sb.material((0.8, 0.8, 0.8, 1)), cull=True, smooth=True)
    if extra_sphere:
        sb.sphere((0.5, 0.5, 0.5), 0.05, sb.material((1, 1, 1, 1)))
    return sb.build()


MESH_MATRIX = np.diag([0.01, 0.01, 0.01, 1.0]).astype(np.float32)  # (the stand-in mesh has a radius of 40)


def test_refusals_create_no_frame(room):
    cam, opt = room["cam"], scenes.options(64, 48, 8, 16)
    mesh, other = binding.Scene(_mesh_room(False), device=0), binding.Scene(_mesh_room(True), device=0)
    try:
        frame = binding.Frame(mesh, cam, opt, base_seed=SEED)
        try:
            _pass(frame)
            blob = frame.checkpoint()
        finally:
            frame.close()
        # another scene: one more sphere
        with pytest.raises(binding.PtError) as refused:
            binding.Frame.restore(other, blob)
        assert refused.value.code == PT_ERR_INVALID and "fingerprint.spheres" in str(refused.value)
        with pytest.raises(binding.PtError) as refused:
            binding.Frame.restore([mesh, other], blob)
        assert refused.value.code == PT_ERR_INVALID and "fingerprint" in str(refused.value)
        # a damaged blob
        damaged = blob.copy()
        damaged[-3] ^= 0x10
        with pytest.raises(binding.PtError) as refused:
            binding.Frame.restore(mesh, damaged)
        assert refused.value.code == PT_ERR_INVALID and "checksum" in str(refused.value)
        # no frame was made and none is counted: both scenes still take a pose (a scene with a live frame refuses one)
        moved = MESH_MATRIX.copy()
        moved[0, 3] = 0.2
        mesh.pose([moved])
        other.pose([moved])
        mesh.pose([MESH_MATRIX])
        # ... and a frame that does load is counted, and counted down when it goes
        loaded = binding.Frame.restore(mesh, blob)
        try:
            with pytest.raises(binding.PtError) as refused:
                mesh.pose([moved])
            assert refused.value.code == PT_ERR_INVALID and "frame" in str(refused.value)
        finally:
            loaded.close()
        mesh.pose([moved])
    finally:
        mesh.close()
        other.close()


# ---- 10. the C++ wrappers ------------------------------------------------------------------------------------------------------------------

def test_cpp_frame_checkpoint(tmp_path):
    exe = str(tmp_path / "frame_checkpoint_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "frame_checkpoint_test.cpp")], exe, extra_flags=["-O1"])
    path = [build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]
    r = subprocess.run([exe], env=dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(path)), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[ OK ]") == 3, r.stdout
