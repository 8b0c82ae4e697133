"""Helpers of the rank tests: a numpy implementation of the semantics in include/word2bits_eval.h ("rank of a given row"),
independent of the C twin -- the scores from bits_testlib.int_scores (1-bit) / codes_testlib.scores (2-bit), the place of
the target counted straight from the definition -- plus the models and questions the tests run on."""
import functools

import numpy as np

import bits_testlib
import codes_testlib

V, Q = 300, 40
# 1-bit: 1024 | 1025 is the boundary between planes in registers and planes in memory
BITS_SIZES = [1, 2, 64, 65, 200, 1024, 1030]
# 2-bit: 416 | 417 is the boundary between two row tiles and one per wavefront, 1217 the first chunked size
CODES_SIZES = [1, 3, 32, 33, 64, 65, 200, 416, 417, 1217]
CASES = [(1, D) for D in BITS_SIZES] + [(2, D) for D in CODES_SIZES]
NAMES = [b"w%d" % i for i in range(V)]


def all_scores(M, bitlevel, b1, b2, b3):
    """[nq, V]: int32 I (1-bit) or the float32 sequence of the codes section (2-bit)"""
    b1, b2, b3 = (np.asarray(x, np.int64) for x in (b1, b2, b3))
    return bits_testlib.int_scores(M, b1, b2, b3) if bitlevel == 1 else codes_testlib.scores(M, b1, b2, b3)


def truth_from_scores(S, bitlevel, D, b1, b2, b3, g):
    """(rank int32 [nq], tied int32 [nq], score float32 [nq]) of target g[q] in question q, by the definition: among the rows
    other than b1, b2, b3 with a score > 0, 1 + the rows with a larger score or the same score and a lower row"""
    nq = S.shape[0]
    rank, tied, score = np.zeros(nq, np.int32), np.zeros(nq, np.int32), np.zeros(nq, np.float32)
    for q in range(nq):
        s, t = S[q], int(g[q])
        if t in (int(b1[q]), int(b2[q]), int(b3[q])) or not s[t] > 0:
            continue
        others = np.ones(S.shape[1], bool)
        others[[b1[q], b2[q], b3[q], t]] = False
        rows = np.arange(S.shape[1])
        rank[q] = 1 + np.count_nonzero(others & ((s > s[t]) | ((s == s[t]) & (rows < t))))
        tied[q] = np.count_nonzero(others & (s == s[t]))
        score[q] = np.float32(s[t]) / np.float32(D) if bitlevel == 1 else s[t]
    return rank, tied, score


def full_list(S, q, b1, b2, b3):
    """the complete answer list of question q: every row other than b1, b2, b3 with a score > 0, in list order"""
    s = S[q].astype(np.float64)
    s[[b1[q], b2[q], b3[q]]] = 0
    idx = np.flatnonzero(s > 0)
    return idx[np.lexsort((idx, -s[idx]))]


def make_case(bitlevel, D):
    """(M, packed, b, g): a "corr" model (its block of identical rows gives ties), Q questions b = int32 [3, Q] (a few with b1
    == b2 == b3) and their targets g: g[0] one of question 0's own rows, g[1] and g[2] inside the block of identical rows"""
    rng = np.random.default_rng(9000 + 10 * D + bitlevel)
    M = bits_testlib.make_signs(rng, "corr", V, D) if bitlevel == 1 else codes_testlib.make_codes(rng, "corr", V, D)
    b = rng.integers(0, V, (3, Q))
    b[:, 2:2 + Q // 8] = b[0, 2:2 + Q // 8]
    g = rng.integers(0, V, Q)
    g[0] = b[1, 0]
    g[1] = V // 3 + 5
    g[2] = V // 3 + 1
    packed = bits_testlib.pack_signs(M) if bitlevel == 1 else codes_testlib.pack_codes(M)
    return M, packed, b.astype(np.int32), g.astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(bitlevel, D):
    """(M, packed, b, g, S, truth): the case, its scores [Q, V] and the numpy truth (rank, tied, score), computed once and
    left unchanged"""
    M, packed, b, g = make_case(bitlevel, D)
    S = all_scores(M, bitlevel, *b)
    truth = truth_from_scores(S, bitlevel, D, *b, g)
    for a in (M, packed, b, g, S) + truth:
        a.setflags(write=False)
    return M, packed, b, g, S, truth


def write_model(path, bitlevel, packed, D):
    lib = bits_testlib if bitlevel == 1 else codes_testlib
    return lib.write_packed_file(path, NAMES, packed, D)


def host_rank(packed, D, bitlevel, b1, b2, b3, g):
    """the C twin for one question: (rc, rank, tied, score); the three outputs start at 77 / 77 / 7.5"""
    from word2bits_amd import _lib
    r, t, s = np.full(1, 77, np.int32), np.full(1, 77, np.int32), np.full(1, 7.5, np.float32)
    rc = _lib.lib().w2b_rank_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0], D, bitlevel, int(b1), int(b2), int(b3), int(g),
                                  r.ctypes.data_as(_lib.i32p), t.ctypes.data_as(_lib.i32p), s.ctypes.data_as(_lib.f32p))
    return rc, int(r[0]), int(t[0]), s[0]


def host_truth(packed, D, bitlevel, b, g):
    """the C twin over a batch: (rank, tied, score) arrays"""
    out = [host_rank(packed, D, bitlevel, *b[:, q], g[q]) for q in range(b.shape[1])]
    assert all(o[0] == 0 for o in out)
    return (np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32),
            np.array([o[3] for o in out], np.float32))


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
