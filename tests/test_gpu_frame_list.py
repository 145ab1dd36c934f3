"""The kernels of pt_frame.hip one launcher at a time on the synthetic lists, records and maps of tests/frame_list_cases.py, through the
test-only probe (tests/hip/frame_list_probe.hip, tests/frame_list_probe.py), against the plain restatement tests/frame_list_ref.py.

Everything compared is an integer or a chain of correctly rounded fp32 operations, so every comparison is exact: equality for integers,
assert_bits_equal for floats.  Two things are left to the device and recorded, not predicted: which place behind the written records the
carry kernel gives a record (frame_list_ref.carry_check says what must hold whatever it gives), and the sign and payload of a NaN rating
(NaN in the same places; the summary's largest error is held to the device's own patterns).

In every call of every test the probe checks the guard bands either side of every device array and the bytes of every array a launcher
takes as const (GuardError, InputChangedError).
"""
import os

import numpy as np
import pytest

from tests import frame_list_cases as fc
from tests import frame_list_ref as fr
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
FILL = 0xDEADBEEF


@pytest.fixture(scope="module")
def probe():
    from tests import frame_list_probe
    p = frame_list_probe.Probe(os.environ.get("PT_FRAME_LIST_PROBE_LIB") or None)  # (another build of the probe: the mutation runs of DESIGN 4.8.1)
    if p.device_count() < 1:
        pytest.fail("no HIP device: the frame list probe has no CPU path")
    return p


def _rule(rule):
    from tests import frame_list_probe
    return frame_list_probe.noise_rule(rule[0], rule[1], rule[2])


def test_constants(probe):
    """The restatement's constants are the headers'."""
    s = probe.sizes()
    assert s["sizeof_park_record"] == 4 * fr.RECORD_WORDS and s["sizeof_estimator"] == 128 and s["offsetof_record_est"] == 4 * fr.EST
    assert s["PT_COMPACT_WORDS"] == fr.COMPACT_WORDS and s["PT_NOISE_SUMMARY_WORDS"] == fr.NOISE_WORDS
    for name in ("FIRST", "SECOND", "LOST", "CARRIED", "WITH_CANDIDATES", "MIN_INVERTED", "MAX", "WITH_RECORD", "WRITTEN", "NO_ROOM", "HELD"):
        assert s["PT_COMPACT_" + name] == getattr(fr, "W_" + name), name
    for name in ("RATED", "UNRATED", "HELD", "MAX_BITS", "FIRST_BIN"):
        assert s["PT_NOISE_" + name] == getattr(fr, "N_" + name), name
    assert (s["PT_STREAM_UNTOUCHED"], s["PT_STREAM_FINISHED"], s["PT_STREAM_PARKED"], s["PT_NO_PARK"]) == (fr.UNTOUCHED, fr.FINISHED, fr.PARKED, fr.NO_PARK)
    assert s["entries_per_block"] == 1024 and s["carry_mark"] == fr.CARRY
    from tests import frame_list_probe as fp
    import ctypes
    assert ctypes.sizeof(fp.NoiseRule) == s["sizeof_noise_rule"] and ctypes.sizeof(fp.DevOptions) == s["sizeof_dev_options"]
    assert fp.DevOptions.stats_sample_count.offset == s["offsetof_stats_sample_count"]
    assert fp.NoiseRule.target.offset == s["offsetof_rule_target"] and fp.NoiseRule.floor.offset == s["offsetof_rule_floor"]


def _run(probe, c, place_only):
    return probe.compact(c["todo"], c["status"], c["parked"], c["park_in"], c["park_out"], c["count0"], c["target"], _rule(c["rule"]), c["resort"], todo_out_fill=FILL,
                         place_only=place_only)


def check_compaction(probe, c):
    what = c["name"]
    parked = c["parked"] if c["parked"] is not None else (c["park_in"] if c["resort"] else c["park_out"])
    want_out, want_status, want_result = fr.compact(c["todo"], c["status"], parked, c["park_in"], c["target"], c["rule"], c["resort"])
    want_blocks = fr.block_counts(c["todo"], c["status"], parked, c["park_in"], c["target"], c["rule"])
    m = len(want_out)
    runs = [_run(probe, c, True), _run(probe, c, True), _run(probe, c, False)]
    for k, got in enumerate(runs):
        w = "%s, run %d" % (what, k)
        assert (got["todo"] == c["todo"]).all() and (got["park_in"] == c["park_in"]).all(), w + ": a const input was written"
        assert c["parked"] is None or (got["parked"] == c["parked"]).all(), w + ": `parked` was written"
        assert (got["block_counts"] == want_blocks).all(), "%s: block counts, first difference in block %s" % (w, np.argwhere(got["block_counts"] != want_blocks)[:1].tolist())
        assert (got["status"] == want_status).all(), "%s: status of stream %d is %d, want %d" % (
            (w,) + tuple(int(a[np.nonzero(got["status"] != want_status)[0][0]]) for a in (np.arange(len(want_status)), got["status"], want_status)))
        assert (got["todo_out"][m:] == FILL).all(), w + ": written behind the new list"
        words = [i for i in range(fr.COMPACT_WORDS) if i != fr.W_NO_ROOM or k < 2]
        assert (got["result"][words] == want_result[words]).all(), "%s: result words %s, want %s" % (w, got["result"].tolist(), want_result.tolist())
    # the place kernel's list, exactly and both times
    for k in (0, 1):
        bad = np.nonzero((runs[k]["todo_out"][:m] != want_out).any(axis=1))[0]
        assert len(bad) == 0, "%s, run %d: %d of %d entries of the new list differ, first at %d: got %s want %s" % (
            what, k, len(bad), m, bad[0], runs[k]["todo_out"][bad[0]].tolist(), want_out[bad[0]].tolist())
        assert (runs[k]["park_out"] == c["park_out"]).all() and runs[k]["park_count"] == c["count0"], what + ": the place kernel moved a record"
    assert (runs[0]["todo_out"] == runs[1]["todo_out"]).all(), what + ": two runs of the place kernel differ"
    # the whole launcher: what the carry did with the marked entries
    full = runs[2]
    if c["target"] > 0 and not c["resort"]:
        fr.carry_check(want_out, full["todo_out"][:m], c["park_in"], c["park_out"], full["park_out"], c["count0"], full["park_count"], c["cap"], full["result"])
    else:
        assert (full["todo_out"][:m] == want_out).all(), what + ": the launcher's list"
        assert full["result"][fr.W_NO_ROOM] == 0 and (full["park_out"] == c["park_out"]).all() and full["park_count"] == c["count0"], what
    return want_result


@pytest.mark.parametrize("mode", sorted(fc.MODES))
def test_compaction(probe, mode):
    """Every pattern of a mode at every length: the list, the status, the block counts and every result word."""
    for c in fc.compact_family(mode):
        check_compaction(probe, c)


@pytest.mark.parametrize("mode", sorted(fc.MODES))
def test_compaction_of_more_blocks_than_threads(probe, mode):
    """264,197 entries in 259 blocks: the place kernel's loop over the block counts takes a second turn."""
    c = fc.big_case(mode)
    result = check_compaction(probe, c)
    assert result[fr.W_FIRST] > 0 and result[fr.W_SECOND] > 0 and (result[fr.W_HELD] > 0) == ("noise" in mode)


def test_hand_written_lists(probe):
    for c, want_out, want_words in fc.hand_written():
        check_compaction(probe, c)
        got = _run(probe, c, True)
        assert (got["todo_out"][:len(want_out)] == want_out).all(), c["name"]
        assert {k: int(got["result"][getattr(fr, "W_" + k)]) for k in want_words} == want_words, c["name"]


def test_carry_without_room(probe):
    """cap = count0 + n_carried - k: exactly k records find no room, their samples are summed, park_count counts on, and nothing is written
    outside park_out's cap records (carry_check; the probe's guard bands)."""
    for c in fc.short_room_cases():
        check_compaction(probe, c)
        got = _run(probe, c, False)
        assert c["count0"] + (len(c["park_in"]) - 2) - c["cap"] > 0, c["name"]
        assert got["result"][fr.W_NO_ROOM] > 0, c["name"]


def test_empty_lists(probe):
    """n = 0 for every launcher: the result words and the summary are zeroed, nothing else is touched."""
    c = fc.compact_case("empty", "progressive_noise", fc.periodic(5, fc.classes_of("progressive_noise")))
    empty = np.zeros((0, 2), U)
    for resort in (False, True):
        got = probe.compact(empty, c["status"], None, c["park_in"], c["park_out"], c["count0"], c["target"], _rule(c["rule"]), resort)
        assert (got["result"] == 0).all() and (got["status"] == c["status"]).all() and (got["park_out"] == c["park_out"]).all() and got["park_count"] == c["count0"]
        assert (got["park_in"] == c["park_in"]).all() and got["todo_out"].size == 0 and got["block_counts"].size == 0
    m = fc.map_case(fc.tile_tables()[2], None, 1, 0.0)
    rule = _rule((1, m["target"], m["floor"]))
    out, summary = probe.rate(empty, m["park"], m["tiles"], m["tile_offset"], m["width"], rule)
    assert out.size == 0 and (summary == 0).all()
    rgba, at = probe.gather(empty, 0, m["park"], m["tiles"], m["tile_offset"], m["width"])
    var, at2 = probe.variance(empty, m["park"], m["tiles"], m["tile_offset"], m["width"], rule.opt)
    assert rgba.size == at.size == var.size == at2.size == 0
    view, samples, emap = np.full((7, 4), 3.5, F), np.full(7, 9, np.int32), np.full(7, 2.5, F)
    got_view, got_samples = probe.scatter(np.zeros((0, 4), F), np.zeros((0, 2), np.int32), view, samples)
    assert_bits_equal(got_view, view, "scatter of nothing")
    assert (got_samples == samples).all()
    assert_bits_equal(probe.noise_scatter(empty, emap), emap, "noise scatter of nothing")
    assert_bits_equal(probe.variance_scatter(np.zeros((0, 4), F), np.zeros(0, np.int32), view), view, "variance scatter of nothing")
    # no pixel at all: the base kernels are not launched
    assert probe.preview_base(np.zeros((0, 4), F), np.zeros(0, np.int32), np.zeros(0, np.uint8))[0].size == 0
    assert probe.noise_base(np.zeros(0, F), np.zeros(0, np.uint8)).size == 0


MAPS = fc.map_family()


@pytest.mark.parametrize("m", MAPS, ids=[m["name"].replace(", ", "-").replace(" ", "_") for m in MAPS])
def test_gather_rate_variance(probe, m):
    """The three one-thread-per-entry kernels on one list: stream_pixel on every tile's first and last stream, the preview colour, the error
    and its summary, the variance."""
    what = m["name"]
    want_rgba, want_at = fr.gather(m["todo"], m["park"], m["tiles"], m["width"])
    rgba, at = probe.gather(m["todo"], 0, m["park"], m["tiles"], m["tile_offset"], m["width"])
    assert (at == want_at).all(), "%s: gather (pixel, samples), first difference at entry %s" % (what, np.argwhere(at != want_at)[:1].tolist())
    assert_bits_equal(rgba, want_rgba, what + ": preview colour")
    want_var, want_pixel = fr.variance(m["todo"], m["park"], m["tiles"], m["width"], m["per_batch"])
    from tests import frame_list_probe as fp
    var, pixel = probe.variance(m["todo"], m["park"], m["tiles"], m["tile_offset"], m["width"], fp.dev_options(m["per_batch"]))
    assert (pixel == want_pixel).all(), what + ": variance pixel"
    assert_bits_equal(var, want_var, what + ": variance")
    for target in (m["target"], F(0.0), F(np.inf)):  # (+inf: no product call sets it, but the rule is stated for it: rated and error <= target)
        rule = (m["per_batch"], target, m["floor"])
        want_out, rated = fr.rate(m["todo"], m["park"], m["tiles"], m["width"], rule)
        out, summary = probe.rate(m["todo"], m["park"], m["tiles"], m["tile_offset"], m["width"], _rule(rule))
        assert (out[:, 0] == want_out[:, 0]).all(), what + ": rating pixel"
        nan = np.isnan(want_out[:, 1].view(F))
        assert np.isnan(out[nan, 1].view(F)).all(), what + ": a NaN rating that is no NaN on the device"
        assert (out[~nan, 1] == want_out[~nan, 1]).all(), "%s: error bits, first difference at entry %s" % (what, np.argwhere(out[:, 1] != want_out[:, 1])[:1].tolist())
        if (nan & rated).any():
            # recorded in DESIGN 4.8.1 and in include/pt_frame_noise.h: a NaN among the rated streams IS the largest error
            assert np.isnan(summary[fr.N_MAX_BITS:fr.N_MAX_BITS + 1].view(F)[0]), what
        want_summary = fr.summary(out[:, 1], rated, target)  # (over the device's own patterns: a NaN's sign and payload are the device's)
        assert (summary == want_summary).all(), "%s, target %g: summary %s, want %s" % (what, target, summary.tolist(), want_summary.tolist())
        if (nan & rated).any() and target == m["target"]:
            print("%s: NaN rating bits %s, summary max bits 0x%08x, its bin %d" % (
                what, sorted(set(hex(b) for b in out[nan, 1].tolist())), summary[fr.N_MAX_BITS], int(np.nonzero(summary[fr.N_FIRST_BIN:])[0].max())))


@pytest.mark.parametrize("n_pixels", fc.PIXEL_COUNTS)
def test_base_and_scatter_kernels(probe, n_pixels):
    """The one-thread-per-pixel base kernels on a cover map of every byte value, and the scatter kernels to distinct pixels that include
    pixel 0 and the last pixel."""
    cover = fc.cover_of(n_pixels)
    rng = np.random.default_rng(n_pixels)
    view, samples = rng.random((n_pixels, 4), dtype=F) + F(1), rng.integers(5, 50, n_pixels).astype(np.int32)
    want_view, want_samples = fr.preview_base(view, samples, cover)
    got_view, got_samples = probe.preview_base(view, samples, cover)
    assert_bits_equal(got_view, want_view, "preview base")
    assert (got_samples == want_samples).all()
    emap = rng.random(n_pixels, dtype=F)
    assert_bits_equal(probe.noise_base(emap, cover), fr.noise_base(cover), "noise base")
    pixels = fc.scatter_pixels(n_pixels, n_pixels)
    assert 0 in pixels and n_pixels - 1 in pixels and len(np.unique(pixels)) == len(pixels)
    n = len(pixels)
    rgba = (rng.random((n, 4), dtype=F) + F(2)).astype(F)
    rgba[0] = [np.inf, -0.0, np.nan, 2.0 ** -140]
    at = np.stack([pixels, rng.integers(1, 99, n)], axis=1).astype(np.int32)
    s_view, s_samples = probe.scatter(rgba, at, want_view, want_samples)
    w_view, w_samples = fr.scatter(rgba, at, want_view, want_samples)
    assert_bits_equal(s_view, w_view, "scatter")
    assert (s_samples == w_samples).all()
    rated = np.stack([pixels.astype(U), rgba[:, :1].view(U)[:, 0]], axis=1)
    assert_bits_equal(probe.noise_scatter(rated, fr.noise_base(cover)), fr.noise_scatter(rated, fr.noise_base(cover)), "noise scatter")
    zeros = np.zeros((n_pixels, 4), F)
    assert_bits_equal(probe.variance_scatter(rgba, pixels, zeros), fr.variance_scatter(rgba, pixels, zeros), "variance scatter")
