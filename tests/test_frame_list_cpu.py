"""Pins tests/frame_list_ref.py (the restatement of the kernels of pt_frame.hip) and tests/frame_list_cases.py (the families the device
tests of tests/test_gpu_frame_list.py are fed) without a GPU: the restatement against a second, deliberately naive statement of the same
rules and against lists written out by hand; stream_pixel against tests/checkpoint_ref.py; the summary against tests/noise_ref.py;
every family against what its docstring claims; and carry_check against hand-made wrong results."""
import numpy as np
import pytest

from tests import checkpoint_ref as ck
from tests import frame_list_cases as fc
from tests import frame_list_ref as fr
from tests import noise_ref as nr

F = np.float32
U = np.uint32
N = fr.NO_PARK


def naive_compact(todo, status, parked, park_in, target, rule, resort):
    """The rule of pt_kernels.h once more, entry by entry, appending to three lists.  Returns what frame_list_ref.compact returns."""
    per_batch, noise_target, floor = rule
    status = [int(s) for s in status]
    first, second, held = [], [], []
    words = dict(LOST=0, CARRIED=0, WITH_CANDIDATES=0, WITH_RECORD=0, WRITTEN=0)
    counts = []
    for stream, y in np.asarray(todo, np.int64).reshape(-1, 2).tolist():
        st = status[stream]
        if st == fr.FINISHED:
            continue
        record, written = None, False
        if st >= fr.PARKED:
            record, written, index = parked[st - fr.PARKED], True, st - fr.PARKED
        elif target > 0 and y != N:
            record, index = park_in[y], (y if resort else y | fr.CARRY)
        elif target <= 0 and y != N:
            words["LOST"] += 1
        samples = 0
        if record is not None:
            samples = int(record[fr.PIXEL_SAMPLE])
            words["WITH_RECORD"] += 1
            words["WRITTEN"] += 1 if written else 0
            words["WITH_CANDIDATES"] += 1 if int(record[fr.N_CANDIDATES]) > 0 else 0
        counts.append(samples)
        words["CARRIED"] += samples
        entry = [stream, index if record is not None else N]
        if target <= 0:
            (first if written else second).append(entry)
        else:
            error = np.inf
            if record is not None:
                error = nr.pixel_error(record[fr.CONTRIBUTION_COUNT:fr.CONTRIBUTION_COUNT + 1].view(np.int32), record[None, fr.MEAN:fr.MEAN + 4].view(F),
                                       record[None, fr.M2:fr.M2 + 4].view(F), per_batch, floor)[0]
            if noise_target > 0 and record is not None and error <= noise_target:
                held.append(entry)
            elif samples < target:
                first.append(entry)
            else:
                second.append(entry)
        status[stream] = fr.UNTOUCHED
    result = np.zeros(fr.COMPACT_WORDS, np.uint64)
    result[fr.W_FIRST], result[fr.W_SECOND], result[fr.W_HELD] = len(first), len(second), len(held)
    for k, v in words.items():
        result[getattr(fr, "W_" + k)] = v
    if counts:
        result[fr.W_MIN_INVERTED], result[fr.W_MAX] = 0xFFFFFFFF - min(counts), max(counts)
    return np.array(first + second + held, np.int64).reshape(-1, 2).astype(U), np.array(status, U), result


def parked_of(c):
    return c["parked"] if c["parked"] is not None else (c["park_in"] if c["resort"] else c["park_out"])


def small_cases(mode):
    return [c for c in fc.compact_family(mode) if len(c["todo"]) <= 257]


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("mode", sorted(fc.MODES))
def test_compact_against_the_naive_statement(mode):
    cases = small_cases(mode) + (fc.short_room_cases(mode) if mode == "progressive_noise" else [])
    assert len(cases) >= 10
    for c in cases:
        got = fr.compact(c["todo"], c["status"], parked_of(c), c["park_in"], c["target"], c["rule"], c["resort"])
        want = naive_compact(c["todo"], c["status"], parked_of(c), c["park_in"], c["target"], c["rule"], c["resort"])
        for g, w, what in zip(got, want, ("list", "status", "result")):
            assert g.shape == w.shape and (g == w).all(), "%s: %s" % (c["name"], what)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_compact_on_hand_written_lists():
    for c, want_out, want_words in fc.hand_written():
        for statement in (fr.compact, naive_compact):
            out, status, result = statement(c["todo"], c["status"], parked_of(c), c["park_in"], c["target"], c["rule"], c["resort"])
            assert (out == want_out).all(), (c["name"], out.tolist())
            assert {k: int(result[getattr(fr, "W_" + k)]) for k in want_words} == want_words, c["name"]
            listed = c["todo"][:, 0]
            finished = c["status"][listed] == fr.FINISHED
            assert (status[listed[~finished]] == fr.UNTOUCHED).all() and (status[listed[finished]] == fr.FINISHED).all()
            others = np.setdiff1d(np.arange(len(status)), listed)
            assert (status[others] == c["status"][others]).all()
    # an 8-entry list of a noise-targeted pass, under resort: held entries last, nothing marked, every record where it was
    templates, target, held = fc.noise_templates(4, fc.DEFAULT_FLOOR)
    rec = fc.blank_records(6, "park_in")
    for row, (name, samples) in enumerate([("exact", 3), ("above", 3), ("below", 9), ("one_batch", 9), ("black", 8), ("overflow", 7)]):
        fc.set_stats(rec, [row], *templates[name])
        rec[row, fr.PIXEL_SAMPLE] = samples
    todo = np.array([[8, 0], [1, 1], [7, N], [3, 2], [2, 3], [6, 4], [5, 5], [4, N]], U)
    for statement in (fr.compact, naive_compact):
        out, status, result = statement(todo, np.zeros(9, U), rec, rec, 8, (4, target, fc.DEFAULT_FLOOR), True)
        #                  first: above (3), none, overflow (7), none       second: one_batch (9)   held: exact, below, black
        assert out.tolist() == [[1, 1], [7, N], [5, 5], [4, N], [2, 3], [8, 0], [3, 2], [6, 4]]
        assert (int(result[fr.W_FIRST]), int(result[fr.W_SECOND]), int(result[fr.W_HELD])) == (4, 1, 3) and result[fr.W_WITH_RECORD] == 6 and result[fr.W_WRITTEN] == 0


@pytest.mark.parametrize("table", fc.tile_tables(), ids=[t[0] for t in fc.tile_tables()])
def test_stream_pixel_against_the_checkpoint_reader(table):
    name, tiles, width, height = table
    assert len(tiles) in (1, 2, 3, 257) and (tiles[:, 2:] > 0).all()
    rows, cols = ck.stream_pixels(tiles)
    streams = fc.tile_streams(tiles)
    assert sorted(streams.tolist()) == list(range(len(rows))), "every stream once"
    first = fr.tile_offsets(tiles).astype(np.int64)
    sizes = tiles[:, 2].astype(np.int64) * tiles[:, 3]
    assert set(first.tolist()) | set((first + sizes - 1).tolist()) <= set(streams[:2 * len(tiles)].tolist()), "the first and last stream of every tile come first"
    got = fr.stream_pixel(streams, tiles, width)
    assert (got == rows[streams] * width + cols[streams]).all()
    assert got.min() >= 0 and got.max() < width * height and len(np.unique(got)) == len(got), "distinct pixels inside the image"
    if len(tiles) > 2:
        assert got.max() == width * height - 1, "a tile ends at the image's last pixel"


def test_tile_tables_hold_the_shapes_claimed():
    shapes = {(int(w), int(h)) for _, tiles, _, _ in fc.tile_tables() for w, h in tiles[:, 2:]}
    assert (1, 1) in shapes and any(w == 1 and h > 1 for w, h in shapes) and any(h == 1 and w > 1 for w, h in shapes)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_summary_against_noise_ref_where_every_rated_error_is_finite():
    checked = 0
    for m in fc.map_family():
        finite = [k for k, name in enumerate(m["names"]) if np.isfinite(fc.template_error(fc.noise_templates(m["per_batch"], m["floor"])[0][name], m["per_batch"], m["floor"]))]
        keep = np.isin(m["rows"], [-1, 0, 1, 2, 3, 4, 5] + [6 + k for k in finite + [m["names"].index("one_batch")]])
        todo = m["todo"][keep]
        for target in (m["target"], F(0)):
            out, rated = fr.rate(todo, m["park"], m["tiles"], m["width"], (m["per_batch"], target, m["floor"]))
            errors = out[:, 1].view(F)
            assert np.isfinite(errors[rated]).all() and np.isinf(errors[~rated]).all()
            got = fr.summary(out[:, 1], rated, target)
            want = nr.summarise(errors, target)
            assert (got[fr.N_RATED], got[fr.N_UNRATED], got[fr.N_HELD]) == (want["streams_rated"], want["streams_unrated"], want["streams_held"])
            assert got[fr.N_MAX_BITS] == F(want["max_error"]).view(U) and (got[fr.N_FIRST_BIN:] == want["histogram"]).all()
            checked += int(rated.sum())
    assert checked > 500


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_noise_templates_rate_as_stated():
    for per_batch, floor in ((1, F(0)), (fc.DEFAULT_PER_BATCH, fc.DEFAULT_FLOOR)):
        t, target, held = fc.noise_templates(per_batch, floor)
        e = {k: fc.template_error(v, per_batch, floor) for k, v in t.items()}
        batches = {k: v[0] // per_batch for k, v in t.items()}
        assert e["exact"].view(U) == target.view(U) and e["below"].view(U) == target.view(U) - 1 and e["above"].view(U) == target.view(U) + 1
        assert e["lower"] < target < e["higher"] and target < e["two_batch"] < np.inf
        assert batches["one_batch"] == 1 and batches["two_batch"] == 2 and batches["black"] == 2 and np.isinf(e["one_batch"])
        assert all(v[0] % per_batch != 0 for v in t.values()) or per_batch == 1
        assert e["overflow"] == np.inf and e["infinite"] == np.inf and batches["overflow"] >= 2 and np.isfinite(t["overflow"][2]).all() and np.isinf(t["infinite"][2][0])
        assert nr.error_bin([e["overflow"]])[0] == 63
        if floor == 0:
            assert np.isnan(e["black"]) and "black" not in held
        else:
            assert e["black"] == 0 and nr.error_bin([e["black"]])[0] == 0 and "black" in held
        with np.errstate(invalid="ignore"):
            assert sorted(held) == sorted(k for k in t if e[k] <= target)


def test_map_cases_hold_what_they_claim():
    for m in fc.map_family():
        rows = m["rows"]
        assert set(rows.tolist()) >= set(range(-1, 6)) or len(rows) < 16, m["name"]
        rec = m["park"][m["todo"][rows >= 0, 1]]
        assert (rec == fc.map_records(m["per_batch"], m["floor"])[0][rows[rows >= 0]]).all()
    rec = fc.map_records(1, 0.0)[0]
    value, collected = rec[:6, fr.PIXEL_VALUE:fr.PIXEL_VALUE + 4].view(F), rec[:6, fr.COLLECTED].view(np.int32)
    assert collected.tolist() == [0, 1, 3, 3, 3, 3] and (value[0] != 0).all()
    tiny = np.finfo(F).tiny
    assert (np.abs(value[3]) < tiny).sum() == 2 and (value[3] > 0).all() and np.isinf(value[4]).any() and np.isnan(value[5]).any()
    assert (rec[:, fr.PIXEL_SAMPLE] != rec[:, fr.COLLECTED]).all(), "a preview colour divided by the wrong count shows"
    lengths = sorted(len(m["todo"]) for m in fc.map_family())
    assert {1, 255, 256, 257} <= set(lengths)


def test_base_and_scatter_cases():
    for n in fc.PIXEL_COUNTS:
        cover = fc.cover_of(n)
        assert set(cover.tolist()) == ({0, 1, 255} if n >= 3 else {0})
        pixels = fc.scatter_pixels(n, n)
        assert 0 in pixels and n - 1 in pixels and len(np.unique(pixels)) == len(pixels) and pixels.min() >= 0 and pixels.max() < n
    assert fc.PIXEL_COUNTS == (1, 255, 256, 257)


def _uninterpreted():
    interpreted = set(range(fr.PIXEL_VALUE, fr.PIXEL_VALUE + 4)) | set(range(fr.MEAN, fr.MEAN + 3)) | set(range(fr.M2, fr.M2 + 3)) | {
        fr.COLLECTED, fr.CONTRIBUTION_COUNT, fr.N_CANDIDATES, fr.PIXEL_SAMPLE}
    return np.array(sorted(set(range(fr.RECORD_WORDS)) - interpreted))


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("mode", sorted(fc.MODES))
def test_compaction_families_hold_what_they_claim(mode):
    target, noise, floor, per_batch, resort = fc.MODES[mode]
    family = fc.compact_family(mode) + [fc.big_case(mode)] + (fc.short_room_cases(mode) if mode == "progressive_noise" else [])
    assert {len(c["todo"]) for c in family} >= set(fc.LENGTHS + fc.CARRY_LENGTHS + (fc.BIG,))
    assert fc.BIG == 264197 and (fc.BIG + 1023) // 1024 > 256
    seen = {c: set() for c in fc.classes_of(mode)}  # class -> positions inside a block
    kinds, sample_sides, counts0, templates_seen = set(), set(), set(), set()
    free = _uninterpreted()
    for c in family:
        n = len(c["todo"])
        cls, where, rec, record = fr.classify(c["todo"], c["status"], parked_of(c), c["park_in"], c["target"], c["rule"])
        assert (cls == c["want"]).all(), c["name"]
        for k in seen:
            seen[k] |= set((np.nonzero(cls == k)[0] % 1024).tolist())
        # streams: distinct, a permutation of a larger range, no entry at its own index (lists of more than a few entries)
        assert len(np.unique(c["todo"][:, 0])) == n and len(c["status"]) > n and c["todo"][:, 0].max() < len(c["status"])
        assert n < 16 or (c["todo"][:, 0] != np.arange(n)).mean() > 0.9
        # record indices: distinct per buffer, below 2^28
        for kind in (fr.R_WRITTEN, fr.R_UNCLAIMED):
            r = rec[where == kind]
            assert len(np.unique(r)) == len(r) and (r < 1 << 28).all(), c["name"]
        assert ((c["todo"][:, 1] == N) | (c["todo"][:, 1] < 1 << 28)).all()
        # words no kernel interprets: unique to their word in their buffer
        for buffer in ("parked", "park_in", "park_out"):
            a = c[buffer]
            if a is not None and len(a) and len(a) < 4000:
                assert len(np.unique(a[:, free])) == a[:, free].size, (c["name"], buffer)
        assert len(np.intersect1d(c["park_in"][:, free], c["park_out"][:, free])) == 0
        if target > 0:
            kinds |= set(np.unique(where[cls != fr.C_FINISHED]).tolist())
            s = record[:, fr.PIXEL_SAMPLE].astype(np.int64)
            sample_sides |= set(np.sign(s[where != fr.R_NONE] - target).tolist())
            counts0.add(c["count0"] > 0)
            templates_seen |= set(np.unique(c["template"][where != fr.R_NONE]).tolist())
            assert c["cap"] == len(c["park_out"]) and (resort or "short" in c["name"] or c["cap"] == c["count0"] + int((where == fr.R_UNCLAIMED).sum()))
        if "big" in c["name"]:
            per_block = fr.block_counts(c["todo"], c["status"], parked_of(c), c["park_in"], c["target"], c["rule"])
            assert len(per_block) == 259 and (per_block[256:, :2].sum(axis=0) > 0).all(), "first and second entries behind block 255"
            assert int((where != fr.R_NONE).sum()) < 3000, "few records"
    if target > 0 and not resort:
        new_lengths = {int((c["want"] != fr.C_FINISHED).sum()) for c in family}
        assert new_lengths >= set(fc.CARRY_LENGTHS), "the list the carry kernel walks: either side of a wavefront's 16 entries and a block's 64"
    for k, positions in seen.items():
        assert {0, 1020, 1021, 1022, 1023} <= positions and {p % 4 for p in positions} == {0, 1, 2, 3}, (mode, k)
    if target > 0:
        assert kinds == ({fr.R_NONE, fr.R_UNCLAIMED} if resort else {fr.R_NONE, fr.R_WRITTEN, fr.R_UNCLAIMED})
        assert sample_sides == {-1, 0, 1} and counts0 == ({False} if resort else {False, True})
        if noise:
            assert templates_seen >= set(fc.noise_templates(per_batch, floor)[0]), templates_seen


def _carried_case():
    c = fc.compact_case("checker", "progressive", fc.periodic(65, fc.classes_of("progressive")), seed=3)
    placed = fr.compact(c["todo"], c["status"], c["park_out"], c["park_in"], c["target"], c["rule"], False)[0]
    marked = fr.carried(placed)
    after, park_out = placed.copy(), c["park_out"].copy()
    after[marked, 1] = c["count0"] + np.arange(marked.sum())[::-1]  # (any order of places is a right result)
    park_out[after[marked, 1]] = c["park_in"][placed[marked, 1] & 0x7FFFFFFF]
    result = np.zeros(fr.COMPACT_WORDS, np.uint64)
    return c, placed, after, park_out, result, int(marked.sum())


def test_carry_check_accepts_a_right_result_and_rejects_wrong_ones():
    c, placed, after, park_out, result, n_carried = _carried_case()
    assert n_carried > 10
    args = lambda a=after, p=park_out, r=result, count=c["count0"] + n_carried: (placed, a, c["park_in"], c["park_out"], p, c["count0"], count, c["cap"], r)
    fr.carry_check(*args())
    marked = np.nonzero(fr.carried(placed))[0]
    twice = after.copy()
    twice[marked[0], 1] = twice[marked[1], 1]  # a duplicated destination
    with pytest.raises(AssertionError):
        fr.carry_check(*args(a=twice))
    one_word = park_out.copy()
    one_word[after[marked[2], 1], 131] ^= 1  # a record with one word changed
    with pytest.raises(AssertionError):
        fr.carry_check(*args(p=one_word))
    other = park_out.copy()
    other[0, 5] ^= 1  # a record that is no destination
    with pytest.raises(AssertionError):
        fr.carry_check(*args(p=other))
    with pytest.raises(AssertionError):
        fr.carry_check(*args(count=c["count0"] + n_carried - 1))
    # too little room: the right result passes, a wrong NO_ROOM sum does not
    short = fc.short_room_cases()[0]
    placed = fr.compact(short["todo"], short["status"], short["park_out"], short["park_in"], short["target"], short["rule"], False)[0]
    marked = np.nonzero(fr.carried(placed))[0]
    after, park_out = placed.copy(), short["park_out"].copy()
    after[marked[:-1], 1] = short["count0"] + np.arange(len(marked) - 1)
    after[marked[-1], 1] = N
    park_out[after[marked[:-1], 1]] = short["park_in"][placed[marked[:-1], 1] & 0x7FFFFFFF]
    result = np.zeros(fr.COMPACT_WORDS, np.uint64)
    result[fr.W_NO_ROOM] = short["park_in"][placed[marked[-1], 1] & 0x7FFFFFFF, fr.PIXEL_SAMPLE]
    args = (placed, after, short["park_in"], short["park_out"], park_out, short["count0"], short["count0"] + len(marked), short["cap"])
    assert short["cap"] == short["count0"] + len(marked) - 1 and result[fr.W_NO_ROOM] > 0
    fr.carry_check(*args, result)
    wrong = result.copy()
    wrong[fr.W_NO_ROOM] += 1
    with pytest.raises(AssertionError):
        fr.carry_check(*args, wrong)
