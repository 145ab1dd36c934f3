"""An independent numpy writer and reader of a frame checkpoint's blob, written from include/pt_checkpoint.h alone (format version 1).
TEST INFRASTRUCTURE ONLY.  tests/test_checkpoint_cpu.py holds the library's writer, parser and kernels against it.

A synthetic STATE is a dict:
    options (5-tuple: width, height, min, max, epsilon), n_views, cameras (V, 17) float32 words of pt_camera_params, seeds (V,) uint64,
    tiles (T, 4) int32 in the frame's order, mode (dict of the header's mode fields), launches, samples_lost, fingerprint (6 counts, 6 words),
    cls (N,) uint8 class per stream in frame stream order, image (rows, width, 4) float32: the caller's image,
    records (N, 132) uint32: the full 528-byte park record of every stream (read only where cls == 2; garbage allowed wherever the format
    says a byte never reaches the blob).
"""
import numpy as np

MAGIC = b"PTFRAME\x1a"
VERSION = 1
FINISHED, UNTOUCHED, RECORD = 0, 1, 2
RECORD_WORDS = 132  # a full park record: stream, cursor, rng[2]; 32 words of estimator; 8 candidates of 12 words
N_CANDIDATES_WORD = 4 + 29  # PtEstimator::n_candidates
PIXEL_SAMPLE_WORD = 4 + 30
EST_PAD_WORD = 4 + 31

OPTIONS = np.dtype([("image_width", "<i4"), ("image_height", "<i4"), ("min_sample_count", "<i4"), ("max_sample_count", "<i4"), ("epsilon", "<f4")])
FINGERPRINT = np.dtype([("counts", "<u8", 6), ("root_box", "<u4", 6)])
HEADER = np.dtype([
    ("magic", "S8"), ("version", "<u4"), ("header_bytes", "<u4"), ("total_bytes", "<u8"),
    ("size_estimator", "<u4"), ("size_candidate", "<u4"), ("max_candidates", "<u4"), ("size_camera", "<u4"), ("size_options", "<u4"),
    ("n_views", "<i4"), ("n_tiles", "<u8"), ("n_streams", "<u8"), ("base_seed", "<u8"),
    ("options", OPTIONS), ("camera", "<u4", 17),
    ("quantum", "<i4"), ("max_passes_per_call", "<i4"), ("passes_completed", "<i4"), ("target", "<i4"), ("pass_in_progress", "<i4"),
    ("noise_target", "<f4"), ("noise_floor", "<f4"), ("noise_fraction", "<f4"),
    ("follow_features", "<i4"), ("feature_max_bounces", "<i4"), ("feature_flags", "<i4"),
    ("launches", "<i4"), ("samples_lost", "<u8"), ("fingerprint", FINGERPRINT),
    ("streams_finished", "<u8"), ("streams_untouched", "<u8"), ("streams_with_record", "<u8"),
    ("bytes_tables", "<u8"), ("bytes_tiles", "<u8"), ("bytes_map", "<u8"), ("bytes_pixels", "<u8"), ("bytes_records", "<u8")])
assert HEADER.itemsize == 352
MODE_FIELDS = ("quantum", "max_passes_per_call", "passes_completed", "target", "pass_in_progress", "noise_target", "noise_floor", "noise_fraction", "follow_features",
               "feature_max_bounces", "feature_flags")
DEFAULT_MODE = dict(quantum=0, max_passes_per_call=0, passes_completed=0, target=0, pass_in_progress=0, noise_target=0.0, noise_floor=1e-5, noise_fraction=1.0,
                    follow_features=0, feature_max_bounces=0, feature_flags=0)


def up16(n):
    return (n + 15) // 16 * 16


def _step(h, v):
    h ^= v
    h = (h * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h ^ (h >> 32)


def checksum(data):
    """Eight interleaved lanes over the little-endian uint64 words: lane l starts as 0xcbf29ce484222325 + l and steps through the words
    i with i % 8 == l; lanes 1..7 are then stepped into lane 0, in order."""
    words = np.frombuffer(data, "<u8")
    lanes = []
    for l in range(8):
        h = 0xcbf29ce484222325 + l
        for w in words[l::8].tolist():
            h = _step(h, w)
        lanes.append(h)
    h = lanes[0]
    for l in range(1, 8):
        h = _step(h, lanes[l])
    return h


def stream_pixels(tiles):
    """(row, column) of every stream of the frame, in frame stream order: tile after tile, row-major inside a tile."""
    rows, cols = [], []
    for x, y, w, h in np.asarray(tiles).reshape(-1, 4).tolist():
        yy, xx = np.mgrid[y:y + h, x:x + w]
        rows.append(yy.ravel())
        cols.append(xx.ravel())
    return (np.concatenate(rows), np.concatenate(cols)) if rows else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def candidates_of(state):
    """n_candidates of every stream that has a record (0 elsewhere), clamped to 0..8 as the library clamps it."""
    cls = np.asarray(state["cls"], np.uint8)
    k = np.clip(np.asarray(state["records"], np.uint32)[:, N_CANDIDATES_WORD].view(np.int32), 0, 8).astype(np.uint8)
    return np.where(cls == RECORD, k, 0).astype(np.uint8)


def map_bytes(state):
    return (np.asarray(state["cls"], np.uint8) | (candidates_of(state) << 2)).astype(np.uint8)


def trimmed_records(state):
    """The records section: per stream with a record (cursor, rng, 0), the estimator with pad 0, k candidates with pad 0."""
    cls = np.asarray(state["cls"], np.uint8)
    k = candidates_of(state)
    out = []
    for s in np.nonzero(cls == RECORD)[0]:
        full = np.asarray(state["records"][s], np.uint32)
        rec = np.zeros(36 + 12 * int(k[s]), np.uint32)
        rec[0:3] = full[1:4]
        rec[4:36] = full[4:36]
        rec[4 + 31] = 0
        for c in range(int(k[s])):
            rec[36 + 12 * c:36 + 12 * c + 9] = full[36 + 12 * c:36 + 12 * c + 9]
        out.append(rec)
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


def header_of(state):
    h = np.zeros((), HEADER)
    h["magic"] = MAGIC
    h["version"], h["header_bytes"] = VERSION, 352
    h["size_estimator"], h["size_candidate"], h["max_candidates"], h["size_camera"], h["size_options"] = 128, 48, 8, 68, 20
    h["n_views"] = state["n_views"]
    h["n_tiles"] = len(state["tiles"])
    h["n_streams"] = len(state["cls"])
    h["base_seed"] = state["seeds"][0]
    h["options"] = np.array(tuple(state["options"]), OPTIONS)
    h["camera"] = np.asarray(state["cameras"], np.float32).reshape(-1, 17)[0].view(np.uint32)
    mode = dict(DEFAULT_MODE, **state.get("mode", {}))
    for f in MODE_FIELDS:
        h[f] = mode[f]
    h["launches"] = state.get("launches", 0)
    h["samples_lost"] = state.get("samples_lost", 0)
    h["fingerprint"]["counts"] = state["fingerprint"][0]
    h["fingerprint"]["root_box"] = state["fingerprint"][1]
    return h


def write(state):
    """The blob of a state, as bytes."""
    cls = np.asarray(state["cls"], np.uint8)
    h = header_of(state)
    v = int(state["n_views"])
    tables = b""
    if v > 1:
        cams = np.asarray(state["cameras"], np.float32).reshape(v, 17).tobytes()
        tables = cams + bytes(up16(len(cams)) - len(cams)) + np.asarray(state["seeds"], "<u8").tobytes()
    tiles = np.asarray(state["tiles"], "<i4").reshape(-1, 4).tobytes()
    rows, cols = stream_pixels(state["tiles"])
    image = np.asarray(state["image"], np.float32).reshape(-1, int(state["options"][0]), 4)
    fin = cls == FINISHED
    pixels = image[rows[fin], cols[fin]].astype("<f4").tobytes()
    records = trimmed_records(state).astype("<u4").tobytes()
    the_map = map_bytes(state).tobytes()
    h["streams_finished"], h["streams_untouched"], h["streams_with_record"] = int(fin.sum()), int((cls == UNTOUCHED).sum()), int((cls == RECORD).sum())
    h["bytes_tables"], h["bytes_tiles"], h["bytes_map"], h["bytes_pixels"], h["bytes_records"] = len(tables), len(tiles), len(the_map), len(pixels), len(records)
    body = b""
    for section in (tables, tiles, the_map, pixels, records):
        body += section + bytes(up16(len(section)) - len(section))
    h["total_bytes"] = 352 + len(body) + 8
    data = h.tobytes() + body
    return data + np.uint64(checksum(data)).tobytes()


def read(blob):
    """A blob back into its parts (no validation beyond the checksum): header, offsets, cameras, seeds, tiles, map, pixels, and the
    trimmed records as a list of uint32 arrays in stream order."""
    data = bytes(blob)
    h = np.frombuffer(data[:352], HEADER)[0]
    at = 352
    off = {}
    for name in ("tables", "tiles", "map", "pixels", "records"):
        off[name] = at
        at = up16(at + int(h["bytes_" + name]))
    off["trailer"] = at
    assert at + 8 == len(data) == int(h["total_bytes"])
    assert checksum(data[:at]) == int(np.frombuffer(data[at:], "<u8")[0])
    v = int(h["n_views"])
    cams = np.frombuffer(data, "<f4", 17 * v, off["tables"]).reshape(v, 17) if v > 1 else h["camera"].view(np.float32).reshape(1, 17)
    seeds = np.frombuffer(data, "<u8", v, up16(off["tables"] + 68 * v)) if v > 1 else np.array([h["base_seed"]], np.uint64)
    tiles = np.frombuffer(data, "<i4", 4 * int(h["n_tiles"]), off["tiles"]).reshape(-1, 4)
    the_map = np.frombuffer(data, np.uint8, int(h["n_streams"]), off["map"])
    pixels = np.frombuffer(data, "<f4", 4 * int(h["streams_finished"]), off["pixels"]).reshape(-1, 4)
    words = np.frombuffer(data, "<u4", int(h["bytes_records"]) // 4, off["records"])
    records, w = [], 0
    for m in the_map[(the_map & 3) == RECORD].tolist():
        n = 36 + 12 * (m >> 2)
        records.append(words[w:w + n])
        w += n
    assert w == len(words)
    return dict(header=h, offsets=off, cameras=cams, seeds=seeds, tiles=tiles, map=the_map, pixels=pixels, records=records)


def inspect(blob):
    """What pt_checkpoint_inspect reports, from the reader."""
    r = read(blob)
    h, m = r["header"], r["map"]
    out = {k: int(h[k]) for k in ("total_bytes", "n_tiles", "n_streams", "streams_finished", "streams_untouched", "streams_with_record", "bytes_tables", "bytes_tiles",
                                  "bytes_map", "bytes_pixels", "bytes_records", "samples_lost", "version", "n_views", "quantum", "max_passes_per_call",
                                  "passes_completed", "target", "pass_in_progress", "follow_features", "launches")}
    out["bytes_header"] = 352
    out["streams_with_candidates"] = int((((m & 3) == RECORD) & ((m >> 2) != 0)).sum())
    assert int(((m & 3) == FINISHED).sum()) == out["streams_finished"] and int(((m & 3) == RECORD).sum()) == out["streams_with_record"]
    for k in ("noise_target", "noise_floor", "noise_fraction"):
        out[k] = float(h[k])
    out["options"] = {k: h["options"][k].item() for k in OPTIONS.names}
    return out


def unpack(state_or_blob, stream_ids=None):
    """What unpack must make of the streams `stream_ids` (frame stream indices in a replica's order; default: all, one replica): the work
    list (records first, then untouched, both in the replica's stream order), the full records with unwritten slots and pads zero, and the
    summary (carried, with_candidates, min, max)."""
    r = read(state_or_blob) if not isinstance(state_or_blob, dict) or "map" not in state_or_blob else state_or_blob
    m = r["map"]
    ids = np.arange(len(m)) if stream_ids is None else np.asarray(stream_ids)
    where = np.cumsum((m & 3) == RECORD) - 1  # the record of a stream, among the blob's
    todo_rec, todo_unt, park = [], [], []
    samples = []
    for local, s in enumerate(ids.tolist()):
        c = m[s] & 3
        if c == RECORD:
            t = r["records"][where[s]]
            full = np.zeros(RECORD_WORDS, np.uint32)
            full[0] = local
            full[1:4] = t[0:3]
            full[4:len(t)] = t[4:]
            todo_rec.append((local, len(park)))
            park.append(full)
            samples.append(int(t[PIXEL_SAMPLE_WORD]))
        elif c == UNTOUCHED:
            todo_unt.append((local, 0xFFFFFFFF))
            samples.append(0)
    todo = np.array(todo_rec + todo_unt, np.uint32).reshape(-1, 2)
    summary = (sum(samples), sum(1 for s in ids.tolist() if (m[s] & 3) == RECORD and (m[s] >> 2)), min(samples) if samples else 0xFFFFFFFF, max(samples) if samples else 0)
    return todo, (np.stack(park) if park else np.zeros((0, RECORD_WORDS), np.uint32)), summary
