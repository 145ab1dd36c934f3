"""A plain numpy restatement of what every kernel of cpupathtrace_amd/csrc/pt_frame.hip is documented to do (pt_kernels.h: the comments of
pt_launch_frame_*; the head comment of pt_frame.hip; pt_noise.h; include/pt_frame_noise.h).  TEST INFRASTRUCTURE ONLY.  Written from
those comments: there are no blocks, no scan and no packed words here.  The new work list is a stable sort of the old one by class.

Layouts: a work list is (n, 2) uint32 (stream, record or NO_PARK); park records are (R, 132) uint32 with the word offsets of
tests/checkpoint_ref.py; a tile table is (T, 4) int32 (x, y, width, height).  Errors use tests/noise_ref.py, variances
tests/denoise_measured_ref.py.  Every float operation is one fp32 operation."""
import numpy as np

from tests import checkpoint_ref as ck
from tests import denoise_measured_ref as dm
from tests import noise_ref as nr

F = np.float32
U = np.uint32
RECORD_WORDS = ck.RECORD_WORDS
EST = ck.N_CANDIDATES_WORD - 29  # the estimator's first word: n_candidates is its 30th
PIXEL_VALUE, MEAN, M2 = EST, EST + 4, EST + 8  # four floats each
COLLECTED, CONTRIBUTION_COUNT = EST + 24, EST + 25
N_CANDIDATES, PIXEL_SAMPLE = ck.N_CANDIDATES_WORD, ck.PIXEL_SAMPLE_WORD

NO_PARK = 0xFFFFFFFF
CARRY = 0x80000000  # "to be carried": bit 31 of an entry's y between the place and the carry kernel
UNTOUCHED, FINISHED, PARKED = 0, 1, 2  # PT_STREAM_*
C_FINISHED, C_FIRST, C_SECOND, C_HELD = 0, 1, 2, 3  # PtEntryClass
R_NONE, R_WRITTEN, R_UNCLAIMED = 0, 1, 2  # PtEntryRecord
COMPACT_WORDS, NOISE_WORDS = 16, 68
W_FIRST, W_SECOND, W_LOST, W_CARRIED, W_WITH_CANDIDATES, W_MIN_INVERTED, W_MAX, W_WITH_RECORD, W_WRITTEN, W_NO_ROOM, W_HELD = range(11)  # PtCompactWord
N_RATED, N_UNRATED, N_HELD, N_MAX_BITS, N_FIRST_BIN = range(5)  # PtNoiseWord


def record_error(records, per_batch, floor):
    """pixel_error of every record (R,) float32"""
    records = np.asarray(records, U).reshape(-1, RECORD_WORDS)
    with np.errstate(over="ignore"):  # (an M2 whose sum overflows is one of the cases)
        return nr.pixel_error(records[:, CONTRIBUTION_COUNT].view(np.int32), records[:, MEAN:MEAN + 4].view(F), records[:, M2:M2 + 4].view(F), per_batch, floor)


def record_rated(records, per_batch):
    records = np.asarray(records, U).reshape(-1, RECORD_WORDS)
    return records[:, CONTRIBUTION_COUNT].view(np.int32) // np.int32(per_batch) >= 2


def classify(todo, status, parked, park_in, target, noise_rule):
    """What the compaction makes of every entry: (class, where its record is, the record's index or NO_PARK, the record itself (n, 132),
    zeros where there is none).  noise_rule: (per_batch, noise_target, floor), noise_target and floor float32."""
    todo = np.asarray(todo, U).reshape(-1, 2)
    status, parked, park_in = np.asarray(status, U), np.asarray(parked, U).reshape(-1, RECORD_WORDS), np.asarray(park_in, U).reshape(-1, RECORD_WORDS)
    n = len(todo)
    st = status[todo[:, 0]]
    finished, written = st == FINISHED, st >= PARKED
    where = np.where(written, R_WRITTEN, R_NONE)
    rec = np.where(written, st - U(PARKED), U(NO_PARK)).astype(U)
    record = np.zeros((n, RECORD_WORDS), U)
    record[written] = parked[rec[written]]
    if target <= 0:  # a plain frame: parked streams first, then untouched ones
        cls = np.where(finished, C_FINISHED, np.where(written, C_FIRST, C_SECOND))
        return cls, where, rec, record
    unclaimed = ~finished & ~written & (todo[:, 1] != NO_PARK)
    where = np.where(unclaimed, R_UNCLAIMED, where)
    rec = np.where(unclaimed, todo[:, 1], rec).astype(U)
    record[unclaimed] = park_in[rec[unclaimed]]
    samples = np.where(where != R_NONE, record[:, PIXEL_SAMPLE].view(np.int32), 0)
    cls = np.where(samples < target, C_FIRST, C_SECOND)
    per_batch, noise_target, floor = noise_rule
    if F(noise_target) > 0:
        with np.errstate(invalid="ignore"):
            held = (where != R_NONE) & (record_error(record, per_batch, floor) <= F(noise_target))  # (a NaN is not at or below anything)
        cls = np.where(held, C_HELD, cls)
    cls = np.where(finished, C_FINISHED, cls)
    where = np.where(finished, R_NONE, where)
    rec = np.where(finished, U(NO_PARK), rec).astype(U)
    record[finished] = 0
    return cls, where, rec, record


def compact(todo, status, parked, park_in, target, noise_rule, resort):
    """The work list after a launch, as the place kernel leaves it (unclaimed records of a progressive frame marked "to be carried"), the
    status afterwards and the result words (NO_ROOM is the carry's: 0 here).  Returns (todo_out (m, 2), status, result (16,) uint64)."""
    todo = np.asarray(todo, U).reshape(-1, 2)
    cls, where, rec, record = classify(todo, status, parked, park_in, target, noise_rule)
    keep = cls != C_FINISHED
    samples = record[:, PIXEL_SAMPLE].astype(np.uint64)  # (the samples the pixel has taken, as the unsigned word the kernel sums)
    if target > 0:
        y = np.where(where == R_WRITTEN, rec, np.where(where == R_UNCLAIMED, rec if resort else rec | U(CARRY), U(NO_PARK))).astype(U)
        has = keep & (where != R_NONE)
        lost = 0
    else:
        y = np.where(cls == C_FIRST, rec, U(NO_PARK)).astype(U)
        has = cls == C_FIRST
        lost = int((keep & (cls == C_SECOND) & (todo[:, 1] != NO_PARK)).sum())
    samples = np.where(has, samples, np.uint64(0))
    order = np.argsort(cls[keep], kind="stable")  # first part, then second, then held, each in the order of `todo`
    out = np.stack([todo[keep, 0], y[keep]], axis=1)[order].astype(U)
    status_after = np.array(status, U)
    status_after[todo[keep, 0]] = UNTOUCHED
    result = np.zeros(COMPACT_WORDS, np.uint64)
    result[W_FIRST], result[W_SECOND], result[W_HELD] = int((cls == C_FIRST).sum()), int((cls == C_SECOND).sum()), int((cls == C_HELD).sum())
    result[W_LOST] = lost
    result[W_CARRIED] = int(samples[keep].sum())
    result[W_WITH_CANDIDATES] = int((has & (record[:, N_CANDIDATES].view(np.int32) > 0)).sum())
    if keep.any():
        result[W_MIN_INVERTED] = 0xFFFFFFFF - int(samples[keep].min())
        result[W_MAX] = int(samples[keep].max())
    result[W_WITH_RECORD] = int(has.sum())
    result[W_WRITTEN] = int((has & (where == R_WRITTEN)).sum())
    return out, status_after, result


def block_counts(todo, status, parked, park_in, target, noise_rule, per_block=1024):
    """(ceil(n / 1024), 3): first, second and held entries of every 1024 entries of `todo`"""
    cls = classify(todo, status, parked, park_in, target, noise_rule)[0]
    n_blocks = (len(cls) + per_block - 1) // per_block
    padded = np.zeros(n_blocks * per_block, np.int64)
    padded[:len(cls)] = cls
    padded = padded.reshape(n_blocks, per_block)
    return np.stack([(padded == c).sum(axis=1) for c in (C_FIRST, C_SECOND, C_HELD)], axis=1).astype(U).reshape(n_blocks, 3)


def carried(todo_after_place):
    y = np.asarray(todo_after_place, U).reshape(-1, 2)[:, 1]
    return (y != NO_PARK) & ((y & U(CARRY)) != 0)


def carry_check(todo_after_place, todo_after_carry, park_in, park_out_before, park_out_after, count0, park_count_after, cap, result):
    """Asserts what the carry kernel must have done.  A checker, not a predictor: the kernel hands out places with an atomic counter."""
    before, after = np.asarray(todo_after_place, U).reshape(-1, 2), np.asarray(todo_after_carry, U).reshape(-1, 2)
    park_in = np.asarray(park_in, U).reshape(-1, RECORD_WORDS)
    out0, out1 = np.asarray(park_out_before, U).reshape(-1, RECORD_WORDS), np.asarray(park_out_after, U).reshape(-1, RECORD_WORDS)
    assert before.shape == after.shape and out0.shape == out1.shape == (cap, RECORD_WORDS)
    marked = carried(before)
    n_carried = int(marked.sum())
    assert (after[:, 0] == before[:, 0]).all(), "the carry changed a stream"
    assert (after[~marked] == before[~marked]).all(), "an entry that was not marked was changed"
    assert park_count_after == count0 + n_carried, "park_count %d, want %d + %d" % (park_count_after, count0, n_carried)
    src = before[marked, 1] & U(~CARRY & 0xFFFFFFFF)
    dst = after[marked, 1]
    placed = dst != NO_PARK
    room = max(0, min(cap, count0 + n_carried) - count0)
    assert int(placed.sum()) == room, "%d records placed, room for %d" % (int(placed.sum()), room)
    got = np.sort(dst[placed])
    assert (got == np.arange(count0, count0 + room, dtype=np.int64)).all(), "the new places are not exactly [%d, %d): %s ..." % (count0, count0 + room, got[:8])
    same = (out1[dst[placed]] == park_in[src[placed]]).all(axis=1)
    assert same.all(), "%d carried records differ from their source, first: entry %d" % (int((~same).sum()), int(np.nonzero(marked)[0][placed][~same][0]))
    others = np.ones(cap, bool)
    others[dst[placed]] = False
    assert (out1[others] == out0[others]).all(), "a record of park_out that is no destination was changed"
    no_room = int(park_in[src[~placed], PIXEL_SAMPLE].view(np.int32).astype(np.int64).sum())
    assert int(np.asarray(result, np.uint64)[W_NO_ROOM]) == no_room, "NO_ROOM %d, want %d" % (int(result[W_NO_ROOM]), no_room)
    assert int((~placed).sum()) == count0 + n_carried - (count0 + room)


# ---- the maps ----------------------------------------------------------------------------------------------------------------------------

def tile_offsets(tiles):
    """The first stream of every tile: streams are dealt tile after tile, one per pixel."""
    tiles = np.asarray(tiles, np.int64).reshape(-1, 4)
    return np.concatenate([[0], np.cumsum(tiles[:, 2] * tiles[:, 3])[:-1]]).astype(U)


def stream_pixel(stream, tiles, width):
    """y * width + x of a stream's pixel: the last tile whose first stream is not behind the stream, row-major inside the tile."""
    tiles = np.asarray(tiles, np.int64).reshape(-1, 4)
    stream = np.asarray(stream, np.int64)
    first = tile_offsets(tiles).astype(np.int64)
    t = np.array([np.nonzero(first <= s)[0][-1] for s in stream.ravel()], np.int64).reshape(stream.shape)
    k = stream - first[t]
    return ((tiles[t, 1] + k // tiles[t, 2]) * width + tiles[t, 0] + k % tiles[t, 2]).astype(np.int32)


def _records_of(todo, park):
    todo, park = np.asarray(todo, U).reshape(-1, 2), np.asarray(park, U).reshape(-1, RECORD_WORDS)
    has = todo[:, 1] != NO_PARK
    record = np.zeros((len(todo), RECORD_WORDS), U)
    record[has] = park[todo[has, 1]]
    return todo, has, record


def gather(todo, park, tiles, width):
    """-> rgba (n, 4): pixel_value * (1 / collected_sample_count) of an entry with a record and collected > 0, else 0; at (n, 2): (pixel,
    pixel_sample of the record, 0 without one)"""
    todo, has, record = _records_of(todo, park)
    collected = record[:, COLLECTED].view(np.int32)
    use = has & (collected > 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = F(1.0) / collected.astype(F)
        rgba = record[:, PIXEL_VALUE:PIXEL_VALUE + 4].view(F) * inv[:, None]
    assert rgba.dtype == F
    rgba = np.where(use[:, None], rgba, F(0.0)).astype(F)
    samples = np.where(has, record[:, PIXEL_SAMPLE].view(np.int32), 0).astype(np.int32)
    return rgba, np.stack([stream_pixel(todo[:, 0], tiles, width), samples], axis=1).astype(np.int32)


def preview_base(view, samples, cover):
    view, samples, cover = np.array(view, F).reshape(-1, 4), np.array(samples, np.int32).reshape(-1), np.asarray(cover, np.uint8).reshape(-1)
    view[cover == 0] = 0
    return view, np.where(cover != 0, -1, 0).astype(np.int32)


def scatter(rgba, at, view, samples):
    view, samples, at = np.array(view, F).reshape(-1, 4), np.array(samples, np.int32).reshape(-1), np.asarray(at, np.int32).reshape(-1, 2)
    view[at[:, 0]] = np.asarray(rgba, F).reshape(-1, 4)
    samples[at[:, 0]] = at[:, 1]
    return view, samples


def rate(todo, park, tiles, width, noise_rule):
    """-> out (n, 2) uint32: (pixel, bits of the error: +inf without a record or with fewer than two batch means), and rated (n,) bool"""
    todo, has, record = _records_of(todo, park)
    per_batch, _, floor = noise_rule
    error = np.where(has, record_error(record, per_batch, floor), F(np.inf)).astype(F)
    out = np.stack([stream_pixel(todo[:, 0], tiles, width).astype(U), error.view(U)], axis=1).astype(U)
    return out, has & record_rated(record, per_batch)


def summary(error_bits, rated, noise_target):
    """The integer reduction of include/pt_frame_noise.h over the bit patterns of the errors: counts of rated and unrated entries, of
    rated ones at or below a target > 0, the largest pattern of a rated entry (as an unsigned word) and rated entries by
    clamp(exponent - 127 + 32, 0, 63).  No pattern is assumed finite."""
    bits, rated = np.asarray(error_bits, U), np.asarray(rated, bool)
    out = np.zeros(NOISE_WORDS, U)
    out[N_RATED], out[N_UNRATED] = int(rated.sum()), int((~rated).sum())
    if F(noise_target) > 0:
        with np.errstate(invalid="ignore"):
            out[N_HELD] = int((rated & (bits.view(F) <= F(noise_target))).sum())
    if rated.any():
        out[N_MAX_BITS] = bits[rated].max()
    exponent = ((bits[rated] >> U(23)) & U(0xFF)).astype(np.int64)
    out[N_FIRST_BIN:] = np.bincount(np.clip(exponent - 127 + 32, 0, 63), minlength=64)
    return out


def noise_base(cover):
    return np.where(np.asarray(cover, np.uint8).reshape(-1) != 0, F(-1.0), F(np.inf)).astype(F)


def noise_scatter(rated, error_map):
    rated, error_map = np.asarray(rated, U).reshape(-1, 2), np.array(error_map, F).reshape(-1)
    error_map.view(U)[rated[:, 0]] = rated[:, 1]
    return error_map


def variance(todo, park, tiles, width, per_batch):
    """-> var (n, 4): pixel_variance of the entry's record, zeros without one; at (n,): the pixel"""
    todo, has, record = _records_of(todo, park)
    var = dm.pixel_variance(record[:, CONTRIBUTION_COUNT].view(np.int32), record[:, M2:M2 + 4].view(F), per_batch)
    return np.where(has[:, None], var, F(0.0)).astype(F), stream_pixel(todo[:, 0], tiles, width)


def variance_scatter(var, at, var_map):
    var_map = np.array(var_map, F).reshape(-1, 4)
    var_map[np.asarray(at, np.int32).reshape(-1)] = np.asarray(var, F).reshape(-1, 4)
    return var_map
