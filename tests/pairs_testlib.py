"""Helpers of the pair-similarity tests (include/word2bits_eval.h, "pair similarity"): the numpy definition of (J, N_A, N_B,
score) on the unpacked integer codes, the host twin, a numpy restatement of the two correlations, and the pairs every test
batch contains."""
import numpy as np

from word2bits_amd import _lib
from bag_testlib import MAX_BAG, make_model, pooled      # noqa: F401  (re-exported for the tests)

ONE = np.array([0x3F800000], np.uint32).view(np.float32)[0]


def flatten_pairs(pairs):
    """[(A, B), ...] -> (ids int32, offsets int64 [2 np + 1])"""
    bags = [np.asarray(x, np.int32) for ab in pairs for x in ab]
    ids = np.concatenate(bags + [np.zeros(0, np.int32)]).astype(np.int32)
    return ids, np.concatenate([[0], np.cumsum([len(b) for b in bags])]).astype(np.int64)


def numpy_pairs(M, pairs):
    """the definition on the integer matrix M [V, D] (+-1, or +-1 / +-3): parts int64 [np, 3] and the score, every double
    operation one numpy float64 operation (multiply, sqrt, divide: each correctly rounded), then one rounding to float32"""
    parts, score = np.zeros((len(pairs), 3), np.int64), np.zeros(len(pairs), np.float32)
    for p, (a, b) in enumerate(pairs):
        TA, TB = pooled(M, a), pooled(M, b)
        J, NA, NB = int(TA @ TB), int(TA @ TA), int(TB @ TB)
        assert max(abs(J), NA, NB) < 2 ** 53
        parts[p] = J, NA, NB
        if NA and NB:
            nn = np.float64(NA) * np.float64(NB)
            score[p] = np.float32(np.float64(J) / np.sqrt(nn))
    return parts, score


def host_pairs(packed, D, bitlevel, ids, offsets, want_score=True, want_parts=True, words=None):
    """w2b_pairs_host: (rc, score float32 [np], parts int64 [np, 3]); an output that was not asked for, or a refused call,
    leaves its fill pattern (NaN / -77)"""
    packed = np.ascontiguousarray(packed, np.uint64)
    ids, offsets = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(offsets, np.int64)
    n = len(offsets) // 2
    score, parts = np.full(n, np.nan, np.float32), np.full((n, 3), -77, np.int64)
    rc = _lib.lib().w2b_pairs_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0] if words is None else words, D, bitlevel,
                                   len(ids), ids.ctypes.data_as(_lib.i32p), n, offsets.ctypes.data_as(_lib.i64p),
                                   score.ctypes.data_as(_lib.f32p) if want_score else None,
                                   parts.ctypes.data_as(_lib.i64p) if want_parts else None)
    return rc, score, parts


def bag_of(rng, V, n):
    """n random ids; bags of 20 ids and more carry padding inside and at both ends, and a repeated id"""
    b = rng.integers(0, V, n).astype(np.int32)
    if n >= 20:
        b[[0, n // 2, n - 1]] = -1
        b[3] = b[2]
    return b


def standard_pairs(rng, V, lengths, totals=()):
    """(pairs, named): every length beside itself, the next one and the third next one; then the special cases, whose indices
    `named` keeps: identical bags, padding, repeats, the three kinds of empty pair, one-word pairs and their near misses; and
    for every t in `totals` pairs of exactly t and t + 1 ids, split evenly and as (t, 1) / (1, t)"""
    L = list(lengths)
    pairs = []
    for i, n in enumerate(L):
        for step in (0, 1, 3):
            pairs.append((bag_of(rng, V, n), bag_of(rng, V, L[(i + step) % len(L)])))
    named = {}

    def add(name, a, b):
        named[name] = len(pairs)
        pairs.append((np.asarray(a, np.int32), np.asarray(b, np.int32)))

    seven = rng.permutation(V)[:7]
    add("identical", seven, seven.copy())
    add("identical_permuted", seven, seven[::-1].copy())
    long_one = bag_of(rng, V, 300)
    add("identical_long", long_one, long_one.copy())
    add("padding", [-1, 5, -1, 9, 9, -1], [-1, -1, 200, 7])
    add("repeats", [7, 7, 7, 30, 7], [30, 30])
    add("empty_no_ids", [], [3])
    add("empty_both", [], [])
    add("empty_padding", [4, 5], [-1, -1, -1])
    add("empty_cancels", [0, 1], [5])                        # row 1 is the opposite of row 0: T == 0 in every column
    add("one_word", [V - 1], [2])
    add("one_word_same", [11], [11])
    add("one_word_opposite", [0], [1])
    add("one_word_and_padding", [V - 1, -1], [2])            # not on the one-word path
    add("one_padding_word", [-1], [2])
    for t in totals:
        add("total_%d_even" % t, bag_of(rng, V, t // 2), bag_of(rng, V, t - t // 2))
        add("total_%d_left" % t, bag_of(rng, V, t - 1), [6])
        add("total_%d_even" % (t + 1), bag_of(rng, V, t // 2), bag_of(rng, V, t + 1 - t // 2))
        add("total_%d_right" % (t + 1), [6], bag_of(rng, V, t))
    pairs += [(rng.integers(0, V, 1).astype(np.int32), rng.integers(0, V, 1).astype(np.int32)) for _ in range(20)]
    return pairs, named


def mean_ranks(v):
    """1-based ranks, equal values sharing the mean of their ranks"""
    v = np.asarray(v, np.float64)
    order = np.argsort(v, kind="stable")
    r = np.empty(len(v), np.float64)
    s = v[order]
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    end = np.concatenate([start[1:], [len(v)]])
    for a, b in zip(start, end):
        r[order[a:b]] = 0.5 * (a + 1 + b)
    return r


def numpy_pearson(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if len(x) < 2:
        return np.nan
    dx, dy = x - x.mean(), y - y.mean()
    sxx, syy = float(dx @ dx), float(dy @ dy)
    if sxx == 0 or syy == 0:
        return np.nan
    return float(dx @ dy) / np.sqrt(sxx * syy)


def numpy_correlations(x, y):
    return numpy_pearson(x, y), numpy_pearson(mean_ranks(x), mean_ranks(y))
