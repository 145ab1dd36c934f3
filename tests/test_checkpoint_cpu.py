"""Checkpoints of a frame (include/pt_checkpoint.h), without a GPU: the blob's writer and parser against an independent
numpy restatement of the format (tests/checkpoint_ref.py), the kernels' per-stream functions compiled for the host on synthetic replicas
(tests/checkpoint_probe.py), the argument checks of the exports, and a stand-alone program that feeds the parser truncated and damaged
blobs under AddressSanitizer and UBSan (tests/cpp/checkpoint_fuzz.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding
from cpupathtrace_amd import build as product
from tests import checkpoint_probe
from tests import checkpoint_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PT_ERR_INVALID = 1
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]  # lane, wavefront and scan-block edges
MIXES = ["finished", "untouched", "records", "mixed"]
WIDTH = 64


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return checkpoint_probe.Probe(checkpoint_probe.build_host(str(tmp_path_factory.mktemp("checkpoint") / "libcheckpoint_probe.so")))


def tiles_of(n):
    """Rectangles of unequal sizes, stacked in an image WIDTH wide, with n pixels in all."""
    shapes = [(7, 3), (64, 2), (5, 5), (1, 1), (13, 1), (32, 4), (3, 9)]
    tiles, y, left, i = [], 0, n, 0
    while left > 0:
        w, h = shapes[i % len(shapes)]
        i += 1
        if w * h > left:
            w, h = min(left, WIDTH), 1
        tiles.append((0 if i % 2 else WIDTH - w, y, w, h))
        y += h
        left -= w * h
    return np.array(tiles, np.int32)


def make_state(n, mix, seed, n_views=1, mode=None):
    """A synthetic frame of n streams: classes by `mix`, n_candidates cycling through 0..8, garbage in every word of a record that no
    reader may depend on -- unwritten candidate slots and the pad words of written ones included."""
    rng = np.random.default_rng(seed)
    tiles = tiles_of(n)
    rows = int(tiles[:, 1].max() + tiles[:, 3][tiles[:, 1].argmax()])
    if mix == "mixed":
        cls = rng.integers(0, 3, n).astype(np.uint8)
    else:
        cls = np.full(n, {"finished": ref.FINISHED, "untouched": ref.UNTOUCHED, "records": ref.RECORD}[mix], np.uint8)
    records = rng.integers(0, 2 ** 32, (n, ref.RECORD_WORDS), dtype=np.uint64).astype(np.uint32)
    records[:, ref.N_CANDIDATES_WORD] = (np.arange(n) + seed) % 9
    records[:, ref.PIXEL_SAMPLE_WORD] = rng.integers(1, 4096, n)
    image = rng.standard_normal((rows, WIDTH, 4)).astype(np.float32)
    cams = rng.standard_normal((n_views, 17)).astype(np.float32)
    seeds = rng.integers(1, 2 ** 63, n_views).astype(np.uint64)
    return dict(options=(WIDTH, rows // n_views if rows % n_views == 0 else rows, 4, 64, 1e-4), n_views=n_views, cameras=cams, seeds=seeds, tiles=tiles,
                mode=mode or {}, launches=3, samples_lost=7, fingerprint=(np.arange(6, dtype=np.uint64) + 10, rng.integers(0, 2 ** 32, 6).astype(np.uint32)),
                cls=cls, image=image, records=records)


def replicas_of(state, n_replicas, seed):
    """The state as n_replicas replicas would hold it: tiles dealt in turn, and per replica its stream ids (frame order), a work list in
    scrambled order and a park buffer with scrambled record indices and unused garbage records between the used ones."""
    rng = np.random.default_rng(seed)
    tiles = state["tiles"]
    first = np.concatenate([[0], np.cumsum(tiles[:, 2].astype(np.int64) * tiles[:, 3])])
    out = []
    for r in range(n_replicas):
        mine = list(range(r, len(tiles), n_replicas))
        ids = np.concatenate([np.arange(first[k], first[k + 1]) for k in mine]) if mine else np.zeros(0, np.int64)
        cls = state["cls"][ids]
        with_record = np.nonzero(cls == ref.RECORD)[0]
        park = rng.integers(0, 2 ** 32, (2 * len(with_record) + 3, ref.RECORD_WORDS), dtype=np.uint64).astype(np.uint32)
        where = rng.permutation(len(park))[:len(with_record)]
        park[where] = state["records"][ids[with_record]]
        park[where, 0] = with_record  # (the record's stream field: the replica's stream)
        todo = [(s, where[i]) for i, s in enumerate(with_record.tolist())] + [(s, 0xFFFFFFFF) for s in np.nonzero(cls == ref.UNTOUCHED)[0].tolist()]
        todo = np.array(todo, np.uint32).reshape(-1, 2)[rng.permutation(len(todo))]
        out.append(dict(tiles=tiles[mine], index=mine, ids=ids, todo=todo, park=park))
    return out


def assemble(state, replicas, packed):
    """The frame-order sections from the replicas' packed ones, by their per-tile offsets, as the host side of a save copies them."""
    n_tiles = len(state["tiles"])
    the_map, pixels, records = [None] * n_tiles, [None] * n_tiles, [None] * n_tiles
    for rep, (m, px, rec, tile_finished, tile_units, totals) in zip(replicas, packed):
        fin = np.concatenate([tile_finished, totals[0:1]]).astype(np.int64)
        units = np.concatenate([tile_units, totals[1:2]]).astype(np.int64)
        first = np.concatenate([[0], np.cumsum(rep["tiles"][:, 2].astype(np.int64) * rep["tiles"][:, 3])])
        for local, k in enumerate(rep["index"]):
            the_map[k] = m[first[local]:first[local + 1]]
            pixels[k] = px[fin[local]:fin[local + 1]]
            records[k] = rec[4 * units[local]:4 * units[local + 1]]
    return np.concatenate(the_map), np.concatenate(pixels), np.concatenate(records)


def test_sizes_of_the_structs():
    assert ref.HEADER.itemsize == binding.CHECKPOINT_HEADER_BYTES == 352
    assert C.sizeof(binding.CheckpointInfo) == 256 and C.sizeof(binding.CheckpointFingerprint) == 72
    header = open(os.path.join(ROOT, "include", "pt_checkpoint.h")).read()
    for name in binding.CHECKPOINT_EXPORTS:
        assert "int %s(" % name in header
    assert not set(binding.CHECKPOINT_EXPORTS) & set(binding.EXPORTS)  # (EXPORTS is what pt_hip.h itself declares)
    assert '#include "pt_checkpoint.h"' in open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert "pt_checkpoint.hip" in product.SOURCES and "pt_checkpoint_format.cpp" in product.SOURCES


@pytest.mark.parametrize("n_views", [1, 3])
def test_writer_and_inspect_against_the_restatement(probe, n_views):
    mode = dict(quantum=8, max_passes_per_call=2, passes_completed=5, target=40, pass_in_progress=1, noise_target=0.02, noise_floor=1e-4, noise_fraction=0.75,
                follow_features=1, feature_max_bounces=6)
    for n, mix in [(1, "records"), (65, "mixed"), (1025, "mixed"), (300, "finished"), (300, "untouched")]:
        state = make_state(n, mix, 11 + n, n_views=n_views, mode=mode)
        want = ref.write(state)
        parts = ref.read(want)
        rc, blob, size = probe.write(state, parts["map"], parts["pixels"], np.concatenate(parts["records"]) if parts["records"] else np.zeros(0, np.uint32))
        assert rc == 0, probe.error()
        assert size == len(want) and blob.tobytes() == want
        rc, info = probe.inspect(want)
        assert rc == 0, probe.error()
        mine = ref.inspect(want)
        for key, value in mine.items():
            if key == "options":
                assert {k: pytest.approx(v) for k, v in value.items()} == info["options"]
            else:
                assert info[key] == pytest.approx(value), key
        assert list(info["fingerprint"]["root_box"]) == list(state["fingerprint"][1]) and info["fingerprint"]["tree_nodes"] == 15
        rc, offsets, per_tile = probe.parse(want, len(state["tiles"]))
        assert rc == 0
        assert [int(o) for o in offsets[2:]] == [parts["offsets"][k] for k in ("tiles", "map", "pixels", "records", "trailer")]
        first = np.concatenate([[0], np.cumsum(state["tiles"][:, 2].astype(np.int64) * state["tiles"][:, 3])])
        assert (per_tile[0] == first).all()
        assert (per_tile[1] == np.concatenate([[0], np.cumsum(state["cls"] == ref.FINISHED)])[first]).all()


@pytest.mark.parametrize("n_replicas", [1, 2, 3])
@pytest.mark.parametrize("mix", MIXES)
def test_pack_and_unpack_on_synthetic_replicas(probe, mix, n_replicas):
    for n in SIZES:
        state = make_state(n, mix, 1000 * n_replicas + n)
        want = ref.write(state)
        parts = ref.read(want)
        replicas = replicas_of(state, n_replicas, n)
        packed = [probe.pack(rep["todo"], rep["park"], len(rep["ids"]), state["image"], rep["tiles"]) for rep in replicas]
        for p in packed:
            assert p[5][2] == 0  # (no entry named a record outside the buffer)
        # the sizes alone are the same sizes
        sized = [probe.pack(rep["todo"], rep["park"], len(rep["ids"]), state["image"], rep["tiles"], sizes_only=True) for rep in replicas]
        for p, q in zip(packed, sized):
            assert (p[0] == q[0]).all() and (p[3] == q[3]).all() and (p[4] == q[4]).all() and (p[5] == q[5]).all()
        rc, blob, _ = probe.write(state, *assemble(state, replicas, packed))
        assert rc == 0, probe.error()
        assert blob.tobytes() == want, (n, mix, n_replicas)
        # unpack(pack(x)) is what the restatement makes of the blob, per replica
        again = []
        for rep, p in zip(replicas, packed):
            todo, park, summary = probe.unpack(p[0], p[2])
            want_todo, want_park, want_summary = ref.unpack(parts, rep["ids"])
            assert (todo == want_todo).all() and (park == want_park).all()
            assert tuple(int(v) for v in summary) == want_summary
            again.append(probe.pack(todo, park, len(rep["ids"]), state["image"], rep["tiles"]))
        # pack(unpack(pack(x))) == pack(x)
        rc, blob2, _ = probe.write(state, *assemble(state, replicas, again))
        assert rc == 0 and blob2.tobytes() == want


def test_a_record_index_outside_the_buffer_reads_nothing(probe):
    state = make_state(65, "records", 5)
    rep = replicas_of(state, 1, 5)[0]
    todo = rep["todo"].copy()
    todo[3, 1] = len(rep["park"]) + 7
    the_map, _, _, _, _, totals = probe.pack(todo, rep["park"], 65, state["image"], rep["tiles"])
    assert totals[2] == 1 and the_map[todo[3, 0]] == ref.UNTOUCHED


def fix_checksum(data):
    data = bytearray(data)
    data[-8:] = np.uint64(ref.checksum(bytes(data[:-8]))).tobytes()
    return bytes(data)


def broken(blob, field, value):
    h = np.frombuffer(blob[:352], ref.HEADER).copy()
    if "." in field:
        a, b = field.split(".")
        h[a][b] = value
    else:
        h[field] = value
    return fix_checksum(h.tobytes() + blob[352:])


def test_every_header_field_broken_in_turn(probe):
    state = make_state(300, "mixed", 3, mode=dict(quantum=4, target=8))
    blob = ref.write(state)
    h = ref.read(blob)["header"]
    assert probe.inspect(blob)[0] == 0
    cases = [("magic", b"XTFRAME\x1a", "magic"), ("version", 2, "version"), ("header_bytes", 360, "header_bytes"), ("total_bytes", int(h["total_bytes"]) + 16, "total_bytes"),
             ("size_estimator", 132, "size_estimator"), ("size_candidate", 52, "size_candidate"), ("max_candidates", 9, "max_candidates"),
             ("size_camera", 72, "size_camera"), ("size_options", 24, "size_options"), ("n_views", 0, "n_views"), ("n_views", 2, "bytes_tables"),
             ("n_tiles", int(h["n_tiles"]) + 1, "n_tiles"), ("n_streams", 301, "n_streams"), ("n_streams", 2 ** 40, "n_streams"),
             ("options.image_width", 0, "options"), ("options.image_height", -4, "options"), ("options.image_width", 8, "tiles"),
             ("quantum", -1, "quantum"), ("max_passes_per_call", -1, "max_passes_per_call"), ("passes_completed", -2, "passes_completed"), ("target", -8, "target"),
             ("pass_in_progress", 2, "pass_in_progress"), ("noise_target", -1.0, "noise_target"), ("noise_target", np.nan, "noise_target"),
             ("noise_floor", np.inf, "noise_floor"), ("noise_fraction", 0.0, "noise_fraction"), ("noise_fraction", 1.5, "noise_fraction"),
             ("follow_features", 2, "follow_features"), ("feature_max_bounces", 33, "feature_params"), ("feature_flags", 1, "feature_params"),
             ("launches", -1, "launches"), ("streams_finished", int(h["streams_finished"]) + 1, "streams_finished"),
             ("streams_untouched", int(h["streams_untouched"]) - 1, "streams_untouched"), ("streams_with_record", int(h["streams_with_record"]) + 1, "streams_with_record"),
             ("bytes_tables", 16, "bytes_tables"), ("bytes_tiles", int(h["bytes_tiles"]) + 16, "bytes_tiles"), ("bytes_map", 299, "bytes_map"),
             ("bytes_pixels", int(h["bytes_pixels"]) + 16, "bytes_pixels"), ("bytes_records", int(h["bytes_records"]) + 48, "bytes_records"),
             ("bytes_records", 2 ** 63, "bytes_records"), ("bytes_tiles", 2 ** 64 - 16, "bytes_tiles")]
    assert {c[0].split(".")[0] for c in cases} >= set(ref.HEADER.names) - {"base_seed", "camera", "samples_lost", "fingerprint", "options"} | {"options"}
    for field, value, named in cases:
        rc, _ = probe.inspect(broken(blob, field, value))
        assert rc == PT_ERR_INVALID, (field, value)
        assert named in probe.error(), (field, value, probe.error())
    # a field any value of which is valid is guarded by the checksum alone
    for field, value in [("base_seed", 99), ("samples_lost", 1), ("passes_completed", 77)]:
        h2 = np.frombuffer(blob[:352], ref.HEADER).copy()
        h2[field] = value
        rc, _ = probe.inspect(h2.tobytes() + blob[352:])
        assert rc == PT_ERR_INVALID and "checksum" in probe.error()
        assert probe.inspect(broken(blob, field, value))[0] == 0
    # ... and the sections behind the header
    parts = ref.read(blob)
    off = parts["offsets"]
    data = bytearray(blob)
    first_record = int(np.nonzero((parts["map"] & 3) == ref.RECORD)[0][0])
    for at, value, named in [(off["map"], 3, "map"), (off["map"], 0x40 | parts["map"][0], "map"), (off["map"] + first_record, ref.RECORD | (9 << 2), "map"),
                             (off["map"] + 300, 1, "padding"), (off["tiles"] + 8, 0, "tiles"), (off["tiles"], 60, "tiles"),
                             (off["records"] + 16 + 116, (parts["map"][first_record] >> 2) ^ 1, "records")]:
        damaged = bytearray(data)
        damaged[at] = value
        rc, _ = probe.inspect(fix_checksum(damaged))
        assert rc == PT_ERR_INVALID and named in probe.error(), (at, value, probe.error())
    flipped = bytearray(data)
    flipped[-1] ^= 0x80
    rc, _ = probe.inspect(bytes(flipped))
    assert rc == PT_ERR_INVALID and "checksum" in probe.error()
    for cut in (0, 8, 351, 352, 359, len(blob) - 1):
        assert probe.inspect(blob[:cut] if cut else b"\0")[0] == PT_ERR_INVALID


def test_capacity_too_small(probe):
    state = make_state(65, "mixed", 9)
    want = ref.write(state)
    parts = ref.read(want)
    records = np.concatenate(parts["records"])
    for capacity in (0, 352, len(want) - 1):
        rc, blob, needed = probe.write(state, parts["map"], parts["pixels"], records, capacity=capacity)
        assert rc == PT_ERR_INVALID and blob is None and needed == len(want) and "capacity" in probe.error()
    rc, blob, _ = probe.write(state, parts["map"], parts["pixels"], records, capacity=len(want) + 100)
    assert rc == 0 and blob.tobytes() == want


def test_argument_checks_of_the_library_without_a_device():
    lib = binding.load()
    for name in binding.CHECKPOINT_EXPORTS:
        assert hasattr(lib, name)
    info = binding.CheckpointInfo()
    blob = np.frombuffer(ref.write(make_state(65, "mixed", 2)), np.uint8)
    assert lib.pt_checkpoint_inspect(None, C.c_size_t(10), C.byref(info)) == PT_ERR_INVALID
    assert lib.pt_checkpoint_inspect(C.c_void_p(blob.ctypes.data), C.c_size_t(len(blob)), None) == PT_ERR_INVALID
    assert lib.pt_checkpoint_inspect(C.c_void_p(blob.ctypes.data), C.c_size_t(len(blob)), C.byref(info)) == 0
    assert binding.checkpoint_inspect(blob)["streams_finished"] == info.streams_finished == int((ref.read(blob.tobytes())["map"] & 3 == 0).sum())
    with pytest.raises(binding.PtError) as e:
        binding.checkpoint_inspect(blob[:-1])
    assert e.value.args and "total_bytes" in str(e.value)
    size, handle, image = C.c_size_t(), C.c_void_p(), np.zeros(4, np.float32)
    assert lib.pt_frame_checkpoint_size(None, C.byref(size)) == PT_ERR_INVALID
    assert lib.pt_frame_checkpoint_save(None, C.c_void_p(image.ctypes.data), C.c_void_p(blob.ctypes.data), C.c_size_t(4), C.byref(size)) == PT_ERR_INVALID
    assert lib.pt_frame_checkpoint_load(None, 1, C.c_void_p(blob.ctypes.data), C.c_size_t(len(blob)), C.c_void_p(image.ctypes.data), C.byref(handle)) == PT_ERR_INVALID
    assert lib.pt_frame_checkpoint_load(None, 1, C.c_void_p(blob.ctypes.data), C.c_size_t(len(blob)), C.c_void_p(image.ctypes.data), None) == PT_ERR_INVALID
    scenes = (C.c_void_p * 1)(None)
    assert lib.pt_frame_checkpoint_load(scenes, 1, C.c_void_p(blob.ctypes.data), C.c_size_t(len(blob)), C.c_void_p(image.ctypes.data), C.byref(handle)) == PT_ERR_INVALID
    assert lib.pt_frame_checkpoint_load(scenes, 0, C.c_void_p(blob.ctypes.data), C.c_size_t(len(blob)), C.c_void_p(image.ctypes.data), C.byref(handle)) == PT_ERR_INVALID
    assert handle.value is None


def test_fuzz_program_under_sanitizers(tmp_path):
    """tests/cpp/checkpoint_fuzz.cpp with pt_checkpoint_format.cpp as an ordinary host program under ASan and UBSan: truncations at
    every length up to the end of the header and a stride beyond, every bit of the header flipped, a fixed-seed sample of bits
    elsewhere; PT_OK or PT_ERR_INVALID every time and a clean exit."""
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = str(tmp_path / "checkpoint_fuzz")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", product.CSRC,
                    os.path.join(HERE, "cpp", "checkpoint_fuzz.cpp"), os.path.join(product.CSRC, "pt_checkpoint_format.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert "checkpoint_fuzz: ok" in done.stdout and "ERROR" not in done.stderr
