"""The per-pixel adaptive estimator of the reference's processItem (src/worker.cpp:149-326) in NumPy, written from that file alone.
TEST INFRASTRUCTURE ONLY.

It stands beside the C oracle (oracle/pt_oracle.c: estimator_reset / _add / _finish) as a second, independent restatement: the compiled
reference cannot be driven with a chosen contribution sequence, so on sequences no render produces (tests/shading_cases.py) the agreement
of the two restatements stands in for it.  float32 arrays, vectorised across sequences; every operation is the reference's, in its order:
  - Color<float> arithmetic is component-wise fp32 (include/PathTrace/util/vector.h), no fused multiply-add;
  - the acceptance ratio of worker.cpp:245 is evaluated in float64 (the literal 1E-5 is a double, so `stddev / (9 * c + 1E-5)` and the
    comparison with 0.2F are carried out in double; `3 * 3 * getContribution(..)` itself is still a float product);
  - std::sort of the qualifying candidates is libstdc++'s __insertion_sort (bits/stl_algo.h), which is what std::sort runs for at most 16
    elements: an element less than the first is rotated to the front, any other is inserted linearly from the back.  With more than 16
    qualifying candidates std::sort would take another route; run() refuses such a sequence instead of guessing.
  - std::max(a, b) is `a < b ? b : a`.

run() also records, per sample, the answer to the question the device asks before a sample starts (may the sample after it begin before
this one is handed over?): yes iff another sample certainly follows under the bound (worker.cpp:193) and the convergence test cannot run
at this one (worker.cpp:239 -- it runs only when a collected sample closes a statistics batch with max(min_sample_count, 2) collected).
"""
import numpy as np

F = np.float32
SORT_INSERTION_MAX = 16  # libstdc++ _S_threshold


def derived_constants(min_sample_count, max_sample_count):
    """worker.cpp:158-164 (C++ int division truncates; every operand here is non-negative or divided after a max with 8)."""
    stats = min(max(min_sample_count // 4, 1), 64)
    batch = max(max(min_sample_count, max_sample_count // 4) // stats, 2)
    d = max_sample_count - min_sample_count
    d8 = -((-d) // 8) if d < 0 else d // 8  # truncation towards zero
    check = min(max(min_sample_count // 2, d8, 8, stats), 1024) // stats
    return stats, batch, check


def closed_candidates_bound(min_sample_count, max_sample_count):
    """How many candidates a pixel can close: every collected sample, max_sample_count of them, worker.cpp:206-222."""
    stats, batch, _ = derived_constants(min_sample_count, max_sample_count)
    batches = max(max_sample_count, 0) // stats
    return (batches - 1) // batch if batches > 0 else 0


def _contribution(c):
    return (c[..., 0] + c[..., 1] + c[..., 2]) / F(3.0)


def run(min_sample_count, max_sample_count, stop_bound, contrib, collected):
    """contrib [n][len][4] float32, collected [n][len]; len >= max_sample_count.  Returns the dict of oracle.Checker.estimator_run (without a
    candidate cap: cand_f [n][K][8], cand_count [n][K] for the K this option pair can close) plus overlap [n][len] (uint8, 0 behind the last
    consumed sample) and first_check [n]: the outcome of the sequence's first convergence test with two batches or more (1 passed, 0 failed,
    -1 none ran), by which the threshold families are checked to reach both sides of their comparison."""
    contrib = np.ascontiguousarray(contrib, dtype=F)
    collected = np.ascontiguousarray(collected).astype(bool)
    n, length = collected.shape
    assert contrib.shape == (n, length, 4) and length >= max_sample_count
    stats, batch, check = derived_constants(min_sample_count, max_sample_count)
    min_needed = max(min_sample_count, 2)
    K = max(closed_candidates_bound(min_sample_count, max_sample_count), 1)

    z4 = lambda: np.zeros((n, 4), F)
    pixel_value, mean, m2, aggregate, cmean, cm2 = z4(), z4(), z4(), z4(), z4(), z4()
    n_collected = np.zeros(n, np.int32)
    count = np.zeros(n, np.int32)
    stats_index = np.zeros(n, np.int32)
    ccount = np.zeros(n, np.int32)
    remaining = np.full(n, check, np.int32)
    n_cand = np.zeros(n, np.int32)
    cand_f = np.zeros((n, K, 8), F)
    cand_count = np.zeros((n, K), np.int32)
    accepted = np.zeros(n, bool)
    consumed = np.zeros(n, np.int32)
    overlap = np.zeros((n, length), np.uint8)
    first_check = np.full(n, -1, np.int32)

    with np.errstate(all="ignore"):
        for i in range(max_sample_count):
            live = ~accepted
            closes = stats_index + 1 == stats
            overlap[:, i] = live & (i + 1 < stop_bound) & ~(closes & (n_collected + 1 >= min_needed))
            consumed[live] = i + 1
            s = np.nonzero(live & collected[:, i])[0]
            if len(s) == 0:
                continue
            c = contrib[s, i]
            count[s] += 1
            stats_index[s] += 1
            aggregate[s] = aggregate[s] + c

            b = s[stats_index[s] == stats]
            if len(b):
                agg = aggregate[b] / F(stats)
                delta = agg - mean[b]
                mean[b] = mean[b] + delta / (count[b] // stats).astype(F)[:, None]
                delta2 = agg - mean[b]
                m2[b] = m2[b] + delta * delta2

                full = b[ccount[b] == batch]
                if len(full):
                    assert (n_cand[full] < K).all(), "more closed candidates than the options allow"
                    cand_f[full, n_cand[full], 0:4] = cmean[full]
                    cand_f[full, n_cand[full], 4:8] = cm2[full]
                    cand_count[full, n_cand[full]] = ccount[full]
                    n_cand[full] += 1
                    cmean[full] = 0
                    cm2[full] = 0
                    ccount[full] = 0

                ccount[b] += 1
                cdelta = agg - cmean[b]
                cmean[b] = cmean[b] + cdelta / ccount[b].astype(F)[:, None]
                cdelta2 = agg - cmean[b]
                cm2[b] = cm2[b] + cdelta * cdelta2

                stats_index[b] = 0
                aggregate[b] = 0

            pixel_value[s] = pixel_value[s] + c
            n_collected[s] += 1

            t = s[(stats_index[s] == 0) & (n_collected[s] >= min_needed)]
            if len(t):
                batches = count[t] // stats
                enough = batches >= 2
                w = m2[t] / (batches - 1).astype(F)[:, None]  # (unused where batches < 2)
                stddev = np.sqrt(w[:, 0] + w[:, 1] + w[:, 2])
                nine_c = F(9.0) * _contribution(mean[t])  # 3 * 3 * getContribution(..): int 9 times float
                ratio = stddev.astype(np.float64) / (nine_c.astype(np.float64) + 1E-5)
                passed = enough & ((stddev < F(1E-4)) | (ratio < np.float64(F(0.2))))
                fresh = enough & (first_check[t] < 0)
                first_check[t[fresh]] = passed[fresh]
                p = t[passed]
                remaining[p] -= 1
                accepted[p[remaining[p] <= 0]] = True
                remaining[t[~passed]] = check

    # worker.cpp:263-319
    value = pixel_value.copy()
    with np.errstate(all="ignore"):
        some = n_collected > 0
        value[some] = pixel_value[some] * (F(1.0) / n_collected[some].astype(F))[:, None]
        min_count = max((batch * 3) // 4, 2)
        for q in np.nonzero(~accepted)[0]:
            cands = [(cand_f[q, j, 0:4], cand_f[q, j, 4:8], int(cand_count[q, j])) for j in range(int(n_cand[q]))]
            if ccount[q] > 0:
                cands.append((cmean[q], cm2[q], int(ccount[q])))
            pcs = []
            for cm, c2, cnt in cands:
                if cnt < min_count:
                    continue
                w = c2 / F(cnt)
                pcs.append((cm.copy(), np.sqrt(F(w[0] + w[1]) + w[2])))
            if not pcs:
                continue
            assert len(pcs) <= SORT_INSERTION_MAX
            for a in range(1, len(pcs)):  # std::__insertion_sort
                val = pcs[a]
                if val[1] < pcs[0][1]:
                    pcs[1:a + 1] = pcs[0:a]
                    pcs[0] = val
                else:
                    j = a
                    while val[1] < pcs[j - 1][1]:  # (unguarded: pcs[0] is not greater than val)
                        pcs[j] = pcs[j - 1]
                        j -= 1
                    pcs[j] = val
            v, stddev = pcs[0][0].copy(), pcs[0][1]
            for a in range(1, len(pcs)):
                other = pcs[a][1]
                x, y = F(stddev + F(0.005)), F(stddev * F(1.01))
                if other < (y if x < y else x):
                    v = v + (pcs[a][0] - v) / F(a + 1)
                    stddev = other
                else:
                    break
            value[q] = v

    est_f = np.concatenate([pixel_value, mean, m2, aggregate, cmean, cm2], axis=1)
    est_i = np.stack([n_collected, count, stats_index, ccount, remaining, n_cand, consumed, np.zeros(n, np.int32)], axis=1).astype(np.int32)
    return {"value": value, "accepted": accepted.astype(np.uint8), "consumed": consumed, "est_f": est_f, "est_i": est_i, "cand_f": cand_f,
            "cand_count": cand_count, "overlap": overlap, "first_check": first_check}
