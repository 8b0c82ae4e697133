"""Helpers of the top-k evaluator tests: the reference's N = k list (ref src/compute-accuracy.c:155-177) from the pinned
top-1 oracle, and a literal transcription of the reference's insertion loop to check that construction against."""
import numpy as np


def oracle_topk(om, b1, b2, b3, k):
    """k rounds of the oracle's top-1 on a copy of om.M in which every row found so far is set to 0: a zero row scores
    0, which never passes `dist > bestd`, and a found row is never b1, b2 or b3, so the query vector is untouched.
    Returns (rows int32 [nq, k], scores float32 [nq, k]); short lists end in -1 / 0."""
    b1, b2, b3 = (np.ascontiguousarray(x, np.int32) for x in (b1, b2, b3))
    nq = len(b1)
    rows, scores = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float32)
    keep = om.M
    try:
        for q in range(nq):
            om.M = keep.copy()
            for j in range(k):
                r, d = om.top1(b1[q:q + 1], b2[q:q + 1], b3[q:q + 1])
                if r[0] < 0:
                    break
                rows[q, j], scores[q, j] = r[0], d[0]
                om.M[r[0]] = 0
    finally:
        om.M = keep
    return rows, scores


def insertion_topk(M, b1, b2, b3, k):
    """ref :155-177 with N = k, two-rounding arithmetic (`dist += vec[a] * M[..]` without contraction), one question."""
    M = np.asarray(M, np.float32)
    words, size = M.shape
    vec = (M[b2] - M[b1]) + M[b3]
    with np.errstate(all="ignore"):
        dist = np.zeros(words, np.float32)
        for a in range(size):                        # every row's chain at once, a = 0..size-1 in order
            dist = dist + vec[a] * M[:, a]
    bestd, bestw = [np.float32(0)] * k, [-1] * k     # ref :164-165
    for c in range(words):
        if c == b1 or c == b2 or c == b3:
            continue
        for a in range(k):                           # ref :166-176
            if dist[c] > bestd[a]:
                for d in range(k - 1, a, -1):
                    bestd[d] = bestd[d - 1]
                    bestw[d] = bestw[d - 1]
                bestd[a] = dist[c]
                bestw[a] = c
                break
    return np.array(bestw, np.int32), np.array(bestd, np.float32)


def seeded_matrix(rng, kind, V, D):
    """the input families of tests/test_gpu_eval.py::test_top1_bit_exact_on_seeded_inputs"""
    if kind == "1bit":
        return (rng.integers(0, 2, (V, D)) * 2 - 1).astype(np.float32) / np.float32(3)
    if kind == "2bit":
        return (rng.choice([.25, .75], (V, D)) * rng.choice([-1, 1], (V, D))).astype(np.float32)
    return (rng.standard_normal((V, D)) * rng.choice([1e-3, 1, 30], (V, 1))).astype(np.float32)


def same_floats(a, b):
    """bit-identical except that any NaN matches any NaN (the rule of tests/test_gpu_eval.py)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]) and np.array_equal(np.isnan(a), np.isnan(b))
