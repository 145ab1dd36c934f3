"""Synthetic work lists, statuses, park records, tile tables and maps for the kernels of pt_frame.hip (tests/frame_list_probe.py runs
them, tests/frame_list_ref.py says what must come out).  TEST INFRASTRUCTURE ONLY.  Every family is a function that returns plain arrays
and says in its docstring what it contains; tests/test_frame_list_cpu.py holds the families to their docstrings.

A compaction CASE is a dict: name, mode, todo (n, 2), status (S,), parked (P, 132) or None (= park_out, as the frame passes it; park_in
under resort), park_in (Q, 132), park_out (cap, 132), count0, cap, target, rule = (per_batch, noise_target float32, floor float32),
resort, want (n,) the class every entry was built to get (frame_list_ref.C_*).

In every case the stream ids are a permutation of a range larger than the list (todo[i].x != i; `status` is indexed by stream and holds
values of its own for the streams outside the list), record indices are permuted too, and every record word that no kernel interprets
holds a value unique to that word of that buffer: a 16-byte unit skipped, duplicated or taken from another record shows."""
import numpy as np

from tests import frame_list_ref as fr
from tests import noise_ref as nr

F = np.float32
U = np.uint32
NO_PARK = fr.NO_PARK
LENGTHS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049)  # either side of a thread's 4 entries, of a block's 1024, and two blocks + 1
CARRY_LENGTHS = (15, 16, 17, 63, 64, 65)  # either side of a wavefront's 16 entries and of a block's 64 in the carry kernel
BIG = 258 * 1024 + 5  # more blocks than the place kernel has threads: its loop over the block counts takes a second turn
TARGET = 8  # the pass's sample count of the progressive cases
DEFAULT_PER_BATCH = nr.stats_sample_count({"min_sample_count": 16})  # 4: stats_sample_count of 16 minimum samples
DEFAULT_FLOOR = F(1e-5)  # pt_frame_set_noise_target's usual floor, the reference's
# mode -> (target, noise target?, floor, per_batch, resort)
MODES = {"plain": (0, False, DEFAULT_FLOOR, DEFAULT_PER_BATCH, False),
         "progressive": (TARGET, False, DEFAULT_FLOOR, DEFAULT_PER_BATCH, False),
         "progressive_noise": (TARGET, True, DEFAULT_FLOOR, DEFAULT_PER_BATCH, False),
         "progressive_noise_floor0": (TARGET, True, F(0.0), 1, False),
         "resort": (TARGET, False, DEFAULT_FLOOR, DEFAULT_PER_BATCH, True),
         "resort_noise": (TARGET, True, DEFAULT_FLOOR, DEFAULT_PER_BATCH, True)}
BUFFER_TAGS = {"parked": 1, "park_in": 2, "park_out": 3, "park": 4}


def classes_of(mode):
    """The classes an entry of a list can get in a mode: nothing is finished when nothing was launched, nothing is held without a target."""
    target, noise, _, _, resort = MODES[mode]
    return ([] if resort else [fr.C_FINISHED]) + [fr.C_FIRST, fr.C_SECOND] + ([fr.C_HELD] if noise else [])


# ---- records -----------------------------------------------------------------------------------------------------------------------------

def blank_records(count, buffer):
    """(count, 132) records whose every word is unique to that word of that buffer: 0xC0000000 | tag << 24 | word number."""
    words = np.arange(count * fr.RECORD_WORDS, dtype=np.int64).reshape(count, fr.RECORD_WORDS)
    assert words.size < 1 << 24
    return (0xC0000000 | (BUFFER_TAGS[buffer] << 24) | words).astype(U)


def set_stats(records, rows, count, mean, m2):
    """The estimator's batch statistics of records[rows]: contribution_count, contribution_mean[0:3], contribution_m2[0:3]"""
    records[rows, fr.CONTRIBUTION_COUNT] = np.asarray(count, np.int32).view(U) if np.ndim(count) else U(count)
    records[rows, fr.MEAN:fr.MEAN + 3] = np.asarray(mean, F).view(U)
    records[rows, fr.M2:fr.M2 + 3] = np.asarray(m2, F).view(U)


def noise_templates(per_batch, floor):
    """Batch statistics (contribution_count, mean (3,), m2 (3,)) by name, and the noise target they are built around:
      exact     three batch means; its pixel_error IS the target, bit for bit: held, because the rule is <=
      below     the same but for a few ulps of m2[0] and mean[0]; its error is one ulp below the target: held
      above     ... one ulp above the target: not held
      lower     a quarter of the m2: well below the target, held
      higher    four times the m2: not held
      one_batch exactly one batch mean: unrated, error +inf, never held
      two_batch exactly two batch means and the m2 of `higher`: rated, not held
      black     two batch means, mean and m2 all zero: at floor 0 it rates 0 / 0 = NaN and is never held; at a floor > 0 it rates 0, lands in
                bin 0 and is held
      overflow  m2 of 3e38 per channel: their sum overflows, the error is +inf though the record is rated: never held, bin 63
      infinite  m2[0] = +inf: the same
    The counts are no multiples of per_batch where per_batch > 1: the division that gives the batch means rounds down.
    Returns (templates, target float32, held: the names a target holds)."""
    extra = 1 if per_batch > 1 else 0
    mean = np.array([0.5, 0.25, 0.125], F)
    m2 = np.array([0.02, 0.03, 0.01], F)
    three = 3 * per_batch + extra
    # exact, below and above: m2[0] and mean[0] moved by a few ulps each around these values, until three records are found whose errors
    # are three consecutive fp32 values (the error's last division steps over some values, so the target is chosen among those reached)
    dm2, dmean = [a.ravel() for a in np.meshgrid(np.arange(-64, 65), np.arange(-16, 17), indexing="ij")]
    m2s, means = np.repeat(m2[None], len(dm2), axis=0), np.repeat(mean[None], len(dm2), axis=0)
    m2s[:, 0] = (m2[:1].view(U).astype(np.int64) + dm2).astype(U).view(F)
    means[:, 0] = (mean[:1].view(U).astype(np.int64) + dmean).astype(U).view(F)
    bits = nr.pixel_error(np.full(len(dm2), three), means, m2s, per_batch, floor).view(U).astype(np.int64)
    reached = np.unique(bits)
    middle = [b for b in reached.tolist() if b - 1 in reached and b + 1 in reached]
    assert middle, "no three consecutive errors"
    at = {name: int(np.nonzero(bits == middle[len(middle) // 2] + d)[0][0]) for name, d in (("below", -1), ("exact", 0), ("above", 1))}
    mean, m2 = means[at["exact"]].copy(), m2s[at["exact"]].copy()
    target = nr.pixel_error([three], mean[None], m2[None], per_batch, floor)[0]
    t = {"exact": (three, mean, m2), "lower": (three, mean, m2 * F(0.25)), "higher": (three, mean, m2 * F(4.0)),
         "one_batch": (per_batch + extra, mean, m2), "two_batch": (2 * per_batch + extra, mean, m2 * F(4.0)),
         "black": (2 * per_batch + extra, np.zeros(3, F), np.zeros(3, F)), "overflow": (three, mean, np.full(3, 3e38, F)),
         "infinite": (three, mean, np.array([np.inf, 0.03, 0.01], F))}
    for name in ("below", "above"):
        t[name] = (three, means[at[name]].copy(), m2s[at[name]].copy())
    held = ["exact", "below", "lower"] + (["black"] if floor > 0 else [])
    return t, F(target), held


def template_error(template, per_batch, floor):
    count, mean, m2 = template
    with np.errstate(over="ignore"):
        return nr.pixel_error([count], np.asarray(mean, F)[None], np.asarray(m2, F)[None], per_batch, floor)[0]


# ---- class patterns ----------------------------------------------------------------------------------------------------------------------

def all_of(n, c):
    return np.full(n, c, np.int64)


def periodic(n, classes, period=7):
    """Period 7, coprime to a thread's 4 entries and a wavefront's 64: every class meets every slot of a thread and both ends of a block."""
    seq = np.array([classes[k % len(classes)] for k in range(period)], np.int64)
    return seq[np.arange(n) % period]


def random_mix(n, classes, seed):
    return np.random.default_rng(seed).choice(np.array(classes, np.int64), size=n)


def solid_run(c, other, tail=5):
    """One block of exactly 1024 entries of class c (a field of the packed scan holds its largest count), a block of another class, a tail"""
    return np.concatenate([all_of(1024, c), all_of(1024, other), all_of(tail, c)])


def last_only(n, c, other):
    """Class c only in the last entry of the last, partial block"""
    p = all_of(n, other)
    p[-1] = c
    return p


def patterns(mode, lengths=LENGTHS + CARRY_LENGTHS):
    """(name, pattern) of a mode: the periodic mix at every length; all of one class, for each class, at 5, 1024 and 1025; the solid runs of
    1024 for each class; random mixes at two seeds (257 and 2049 entries); each class alone in the last entry of a partial block (1025 and
    2049 entries); only finished entries (5 and 1025; not under resort, where nothing is finished)."""
    classes = classes_of(mode)
    out = [("periodic %d" % n, periodic(n, classes)) for n in lengths]
    for c in classes:
        other = classes[(classes.index(c) + 1) % len(classes)]
        out += [("all class %d, %d" % (c, n), all_of(n, c)) for n in (5, 1024, 1025)]
        out.append(("solid run of class %d" % c, solid_run(c, other)))
        out += [("class %d last only, %d" % (c, n), last_only(n, c, other)) for n in (1025, 2049)]
    out += [("random %d seed %d" % (n, seed), random_mix(n, classes, seed)) for n, seed in ((257, 1), (2049, 2))]
    return out


def big_pattern(mode):
    """BIG entries: every 97th has a record (those cycle through the classes that need one), every 5th of the others is finished (under
    resort: none), the rest have none: untouched streams of a plain frame, streams without a sample of a progressive one.  Returns the
    pattern and which entries have a record."""
    target, noise, _, _, resort = MODES[mode]
    i = np.arange(BIG)
    with_record = i % 97 == 0
    if target <= 0:
        p = np.where(with_record, fr.C_FIRST, np.where(i % 5 == 0, fr.C_FINISHED, fr.C_SECOND))
    else:
        cyc = np.array([fr.C_SECOND, fr.C_HELD, fr.C_FIRST] if noise else [fr.C_SECOND, fr.C_FIRST], np.int64)
        p = np.where(with_record, cyc[(i // 97) % len(cyc)], np.where((i % 5 == 0) & (not resort), fr.C_FINISHED, fr.C_FIRST))
    return p.astype(np.int64), with_record


# ---- compaction cases --------------------------------------------------------------------------------------------------------------------

def compact_case(name, mode, pattern, seed=0, with_record=None, count0_zero=False, room_short=0):
    """A list whose entry i the compaction must give class pattern[i] in `mode`.
    plain: finished = status FINISHED; first = status PARKED + r with the records r a permutation, in a `parked` buffer of its own, sample
      counts (7 i) % 23 and 0, 1 or 2 candidates; second = status UNTOUCHED, every third of them still naming an earlier record (LOST).
    progressive: first = fewer samples than TARGET (1 or TARGET - 1 with a record, or no record at all), second = TARGET, TARGET + 1 or
      TARGET + 5 samples, held (noise modes) = a record one of the held templates of noise_templates() fills, with 1, TARGET - 1, TARGET or
      TARGET + 3 samples; first and second entries of the noise modes take the templates a target does not hold, in turn.  A record is
      WRITTEN (status PARKED + r, r < count0, in park_out, which is also `parked`) or UNCLAIMED (status UNTOUCHED, todo.y = its index in
      park_in); under resort and with count0_zero every record is unclaimed.  count0 counts 3 written records no entry names as well.
      park_out has room for every unclaimed record less room_short.
    with_record (n,) bool: which first entries may have a record (default: two in three)."""
    target, noise, floor, per_batch, resort = MODES[mode]
    pattern = np.asarray(pattern, np.int64)
    n = len(pattern)
    rng = np.random.default_rng(1000 + seed)
    n_streams = n + n // 2 + 7
    todo = np.zeros((n, 2), U)
    todo[:, 0] = rng.permutation(n_streams)[:n]
    status = (0x5A000000 + np.arange(n_streams)).astype(U)  # (streams outside the list: a value of their own each, which must stay)
    i = np.arange(n)
    finished = pattern == fr.C_FINISHED
    assert set(np.unique(pattern).tolist()) <= set(classes_of(mode)), (mode, np.unique(pattern))
    templates, noise_target, held_names = noise_templates(per_batch, floor)
    rule = (per_batch, noise_target if noise else F(0.0), floor)
    case = dict(name="%s: %s" % (mode, name), mode=mode, target=target, rule=rule, resort=resort, want=pattern)
    if target <= 0:
        first, second = pattern == fr.C_FIRST, pattern == fr.C_SECOND
        n_first = int(first.sum())
        parked = blank_records(n_first + 2, "parked")
        r = rng.permutation(n_first + 2)[:n_first]
        status[todo[finished, 0]] = fr.FINISHED
        status[todo[first, 0]] = fr.PARKED + r
        status[todo[second, 0]] = fr.UNTOUCHED
        parked[r, fr.PIXEL_SAMPLE] = (7 * i[first]) % 23
        parked[r, fr.N_CANDIDATES] = i[first] % 3
        parked[:, fr.PIXEL_VALUE:fr.PIXEL_VALUE + 4] = F(0.5).view(U)
        set_stats(parked, slice(None), 3 * per_batch, templates["exact"][1], templates["exact"][2])
        todo[:, 1] = np.where(i % 3 == 0, U(0x100) + i.astype(U), U(NO_PARK))  # (an earlier launch's record: no kernel follows it in a plain frame)
        case.update(todo=todo, status=status, parked=parked, park_in=blank_records(1, "park_in"), park_out=np.zeros((0, fr.RECORD_WORDS), U), count0=0, cap=0)
        return case
    # which entries have a record, and where
    pick = rng.integers(0, 3, n)
    may = np.ones(n, bool) if with_record is None else np.asarray(with_record, bool)
    has = ~finished & ((pattern != fr.C_FIRST) | ((pick != 2) & may))
    assert with_record is None or not (has & ~may).any(), "a class that needs a record where none is allowed"
    written = has & (pick == 0) & (not resort) & (not count0_zero)
    unclaimed = has & ~written
    # samples and statistics
    samples = np.zeros(n, np.int64)
    pick2 = rng.integers(0, 12, n)
    samples = np.where(pattern == fr.C_FIRST, np.array([1, TARGET - 1])[pick2 % 2], samples)
    samples = np.where(pattern == fr.C_SECOND, np.array([TARGET, TARGET + 1, TARGET + 5])[pick2 % 3], samples)
    samples = np.where(pattern == fr.C_HELD, np.array([1, TARGET - 1, TARGET, TARGET + 3])[pick2 % 4], samples)
    not_held = [k for k in templates if k not in held_names]
    names = np.array(sorted(templates))
    turn = np.cumsum(has) - 1
    which = np.where(pattern == fr.C_HELD, np.array([sorted(templates).index(k) for k in held_names])[turn % len(held_names)],
                     np.array([sorted(templates).index(k) for k in not_held])[turn % len(not_held)])
    n_written, n_unclaimed = int(written.sum()), int(unclaimed.sum())
    count0 = 0 if (resort or count0_zero) else n_written + 3
    cap = 0 if resort else max(count0, count0 + n_unclaimed - room_short)
    park_in, park_out = blank_records(n_unclaimed + 2, "park_in"), blank_records(cap, "park_out")
    r_written, r_in = rng.permutation(count0)[:n_written], rng.permutation(n_unclaimed + 2)
    r_unclaimed, spare = r_in[:n_unclaimed], r_in[n_unclaimed:]  # (two records of park_in that no unclaimed entry names)
    status[todo[finished, 0]] = fr.FINISHED
    status[todo[~finished, 0]] = fr.UNTOUCHED
    status[todo[written, 0]] = fr.PARKED + r_written
    todo[:, 1] = np.where(i % 2 == 0, U(spare[0]), U(NO_PARK))  # (a claimed or finished stream: the record it was started from, or none)
    todo[~finished & ~has, 1] = NO_PARK
    todo[unclaimed, 1] = r_unclaimed
    for buffer, rows, sel in ((park_out, r_written, written), (park_in, r_unclaimed, unclaimed)):
        buffer[rows, fr.PIXEL_SAMPLE] = samples[sel]
        buffer[rows, fr.N_CANDIDATES] = i[sel] % 3
        buffer[rows, fr.COLLECTED] = np.maximum(samples[sel] - 1, 0)
        buffer[rows, fr.PIXEL_VALUE:fr.PIXEL_VALUE + 4] = (F(0.25) * (1 + i[sel] % 5).astype(F))[:, None].repeat(4, axis=1).view(U)
        for k, name_k in enumerate(names):
            m = which[sel] == k
            set_stats(buffer, rows[m], templates[name_k][0], templates[name_k][1], templates[name_k][2])
    case.update(todo=todo, status=status, parked=None, park_in=park_in, park_out=park_out, count0=count0, cap=cap, template=np.where(has, names[which], ""))
    return case


def compact_family(mode):
    """Every pattern of patterns(mode) as a case; in the progressive modes the periodic cases of 17, 65, 257 and 2049 entries once more with
    count0 = 0 (no written record), and periodic cases without finished entries at CARRY_LENGTHS, so that the NEW list, which the carry kernel
    walks, has these lengths."""
    out = [compact_case(name, mode, p, seed=k) for k, (name, p) in enumerate(patterns(mode))]
    target, _, _, _, resort = MODES[mode]
    if target > 0 and not resort:
        out += [compact_case("periodic %d, count0 = 0" % n, mode, periodic(n, classes_of(mode)), seed=100 + n, count0_zero=True) for n in (17, 65, 257, 2049)]
        unfinished = [c for c in classes_of(mode) if c != fr.C_FINISHED]
        out += [compact_case("periodic %d, nothing finished" % n, mode, periodic(n, unfinished), seed=200 + n) for n in CARRY_LENGTHS]
    return out


def big_case(mode):
    """The BIG list of big_pattern(mode): 264,197 entries in 259 blocks, 2,724 of them with a record."""
    p, with_record = big_pattern(mode)
    return compact_case("big", mode, p, seed=7, with_record=with_record)


def short_room_cases(mode="progressive_noise"):
    """Too little room in park_out for the carry: the periodic list of 257 entries with cap = count0 + n_carried - k for k = 1 and for
    k = n_carried (no room at all), with count0 > 0 and with count0 = 0.  Every write stays inside park_out's cap records."""
    out = []
    for count0_zero in (False, True):
        base = compact_case("", mode, periodic(257, classes_of(mode)), seed=55, count0_zero=count0_zero)
        n_carried = len(base["park_in"]) - 2
        for k in (1, n_carried):
            out.append(compact_case("room short by %d of %d, count0 %s 0" % (k, n_carried, "=" if count0_zero else ">"), mode, periodic(257, classes_of(mode)), seed=55,
                                    count0_zero=count0_zero, room_short=k))
    return out


def hand_written():
    """Lists of at most 8 entries with their expected result written out: (case fields, expected todo_out, expected result words by name)"""
    N = NO_PARK
    rec = blank_records(4, "parked")
    rec[:, fr.PIXEL_SAMPLE] = [5, 9, 2, 7]
    rec[:, fr.N_CANDIDATES] = [0, 2, 0, 1]
    plain = dict(name="hand: plain", mode="plain", target=0, rule=(4, F(0), DEFAULT_FLOOR), resort=False,
                 # streams      30 untouched(lost) 31 parked r2   32 finished  33 untouched  34 parked r0  35 untouched(lost)
                 todo=np.array([[30, 1], [31, N], [32, 3], [33, N], [34, 0], [35, 2]], U),
                 status=np.concatenate([np.full(30, 77, U), np.array([0, 2 + 2, 1, 0, 2 + 0, 0], U)]),
                 parked=rec, park_in=blank_records(1, "park_in"), park_out=np.zeros((0, fr.RECORD_WORDS), U), count0=0, cap=0)
    plain_out = np.array([[31, 2], [34, 0], [30, N], [33, N], [35, N]], U)
    plain_words = dict(FIRST=2, SECOND=3, LOST=2, CARRIED=2 + 5, WITH_CANDIDATES=0, MIN_INVERTED=0xFFFFFFFF - 0, MAX=5, WITH_RECORD=2, WRITTEN=2, NO_ROOM=0, HELD=0)
    out_rec, in_rec = blank_records(3, "park_out"), blank_records(3, "park_in")
    out_rec[:, fr.PIXEL_SAMPLE] = [8, 3, 99]
    out_rec[:, fr.N_CANDIDATES] = [1, 0, 5]
    in_rec[:, fr.PIXEL_SAMPLE] = [9, 7, 8]
    in_rec[:, fr.N_CANDIDATES] = [0, 3, 0]
    C = fr.CARRY
    prog = dict(name="hand: progressive", mode="progressive", target=8, rule=(4, F(0), DEFAULT_FLOOR), resort=False,
                # streams    10 written r0 (8: second)  11 no record (first)  12 unclaimed r1 (7: first)  13 finished  14 written r1 (3: first)
                #            15 unclaimed r2 (8: second)  16 unclaimed r0 (9: second)
                todo=np.array([[10, 2], [11, N], [12, 1], [13, 0], [14, N], [15, 2], [16, 0]], U),
                status=np.concatenate([np.full(10, 55, U), np.array([2 + 0, 0, 0, 1, 2 + 1, 0, 0], U)]),
                parked=None, park_in=in_rec, park_out=np.concatenate([out_rec[:2], blank_records(5, "park_out")[2:]]), count0=2, cap=5)
    prog_out = np.array([[11, N], [12, 1 | C], [14, 1], [10, 0], [15, 2 | C], [16, 0 | C]], U)
    prog_words = dict(FIRST=3, SECOND=3, LOST=0, CARRIED=8 + 0 + 7 + 3 + 8 + 9, WITH_CANDIDATES=2, MIN_INVERTED=0xFFFFFFFF - 0, MAX=9, WITH_RECORD=5, WRITTEN=2, NO_ROOM=0,
                      HELD=0)
    return [(plain, plain_out, plain_words), (prog, prog_out, prog_words)]


# ---- tile tables and map cases -----------------------------------------------------------------------------------------------------------

def tile_tables():
    """(name, tiles (T, 4), image width, image height): 1, 2, 3 and 257 tiles, no tile of zero area.
      one tile     a 5 x 3 tile inside a 16 x 8 image
      two tiles    a 1 x 1 tile, then a tile one pixel wide (1 x 4)
      three tiles  a tile one pixel high (6 x 1), a 1 x 1 tile, and a 3 x 2 tile that ends at the image's last pixel
      257 tiles    cells of 2 x 2 pixels, 20 to a row of a 40 x 26 image; tile k has width 1 + k % 2 and height 1 + (k // 2) % 2; the last
                   one is a 2 x 2 tile that ends at the image's last pixel"""
    many = [[2 * (k % 20), 2 * (k // 20), 1 + k % 2, 1 + (k // 2) % 2] for k in range(256)] + [[38, 24, 2, 2]]
    return [("one tile", np.array([[2, 1, 5, 3]], np.int32), 16, 8),
            ("two tiles", np.array([[3, 0, 1, 1], [7, 2, 1, 4]], np.int32), 9, 7),
            ("three tiles", np.array([[1, 0, 6, 1], [0, 2, 1, 1], [5, 3, 3, 2]], np.int32), 8, 5),
            ("257 tiles", np.array(many, np.int32), 40, 26)]


def tile_streams(tiles, seed=0):
    """Every stream of a tile table in an order that starts with the first and the last stream of every tile and goes on with the others,
    shuffled"""
    first = fr.tile_offsets(tiles).astype(np.int64)
    sizes = np.asarray(tiles, np.int64)[:, 2] * np.asarray(tiles, np.int64)[:, 3]
    ends = np.unique(np.concatenate([first, first + sizes - 1]))
    rest = np.setdiff1d(np.arange(int(sizes.sum())), ends)
    return np.concatenate([ends, np.random.default_rng(seed).permutation(rest)]).astype(U)


def map_records(per_batch, floor):
    """The records of a map case, by row: 0..5 for the gather -- collected_sample_count 0 with a pixel_value that is not zero (colour 0, the
    samples as recorded), 1, 3, a pixel_value holding a denormal (2^-140) with 3 collected, one holding +inf, one holding a NaN and a
    negative value; 6.. one record per template of noise_templates(per_batch, floor), in the order of sorted names.  Returns (records,
    names of rows 6.., noise target, held names)."""
    templates, target, held = noise_templates(per_batch, floor)
    names = sorted(templates)
    rec = blank_records(6 + len(names), "park")
    rec[:, fr.PIXEL_SAMPLE] = 3 + np.arange(len(rec))
    rec[:, fr.N_CANDIDATES] = 0
    values = np.array([[0.5, 1.5, 2.5, 1.0], [0.1, 0.2, 0.3, 1.0], [3.0, 1.0, 10.0, 3.0], [2.0 ** -140, 1.0, 2.0 ** -149, 3.0], [np.inf, 1.0, 2.0, 3.0],
                       [np.nan, -1.0, 0.0, 3.0]], F)
    rec[:6, fr.PIXEL_VALUE:fr.PIXEL_VALUE + 4] = values.view(U)
    rec[6:, fr.PIXEL_VALUE:fr.PIXEL_VALUE + 4] = np.array([1.0, 2.0, 4.0, 7.0], F).view(U)
    rec[:, fr.COLLECTED] = [0, 1, 3, 3, 3, 3] + [7] * len(names)
    set_stats(rec, slice(0, 6), 3 * per_batch, templates["exact"][1], templates["exact"][2])
    for k, name in enumerate(names):
        set_stats(rec, [6 + k], *templates[name])
    return rec, names, target, held


def map_case(table, n, per_batch, floor, seed=0):
    """A work list of the first n streams of tile_streams(table) (all of them for n = None); entry i has no record when i % 4 == 3, else
    a record of map_records() -- the rows in turn, through a permutation, several entries sharing one row of a short table."""
    name, tiles, width, height = table
    streams = tile_streams(tiles, seed)
    streams = streams if n is None else streams[:n]
    rec, names, target, held = map_records(per_batch, floor)
    perm = np.random.default_rng(seed).permutation(len(rec))
    # the records as the list finds them: shuffled, so that row != order
    park = rec[np.argsort(perm)]  # row perm[k] of park is rec[k]
    i = np.arange(len(streams))
    y = np.where(i % 4 == 3, NO_PARK, perm[(i - i // 4) % len(rec)]).astype(U)
    todo = np.stack([streams, y], axis=1).astype(U)
    return dict(name="%s, %d entries, batches of %d, floor %g" % (name, len(todo), per_batch, floor), todo=todo, park=park, tiles=tiles,
                tile_offset=fr.tile_offsets(tiles), width=width, height=height, per_batch=per_batch, floor=F(floor), target=target,
                rows=np.where(y == NO_PARK, -1, np.argsort(perm)[np.where(y == NO_PARK, 0, y)]), names=names, held=held)


def map_family():
    """Every tile table with all of its streams, at stats_sample_count 1 with floor 0 and at the default with the default floor; the 257-tile
    table also with lists of 1, 255, 256 and 257 entries (either side of the one-thread-per-entry kernels' block of 256)."""
    tables = tile_tables()
    out = []
    for per_batch, floor in ((1, 0.0), (DEFAULT_PER_BATCH, float(DEFAULT_FLOOR))):
        out += [map_case(t, None, per_batch, floor, seed=k) for k, t in enumerate(tables)]
        out += [map_case(tables[3], n, per_batch, floor, seed=10 + n) for n in (1, 255, 256, 257)]
    return out


PIXEL_COUNTS = (1, 255, 256, 257)


def cover_of(n_pixels):
    """A cover map with every byte value that occurs: 0, 1, 255, in turn (period 3)"""
    return np.array([0, 1, 255], np.uint8)[np.arange(n_pixels) % 3]


def scatter_pixels(n_pixels, seed=0):
    """Distinct pixels of a map to scatter to: pixel 0, the last pixel, and every second of the others in a shuffled order"""
    inner = np.random.default_rng(seed).permutation(np.arange(1, max(n_pixels - 1, 1)))[::2]
    pixels = np.unique(np.concatenate([[0, n_pixels - 1], inner]))
    return np.random.default_rng(seed + 1).permutation(pixels).astype(np.int32)
