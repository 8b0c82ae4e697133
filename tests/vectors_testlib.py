"""Helpers of the vector-question tests (include/word2bits_eval.h, "vector questions"): the host twin, an independent numpy
chain it is checked against, the answer lists that scores of every row imply, and the queries every GPU batch contains."""
import numpy as np

from word2bits_amd import _lib
import codes_testlib
from bag_testlib import answer_list, make_model   # noqa: F401  (make_model: re-exported for the tests)


def host_vector(packed, D, bitlevel, x, normalize):
    """w2b_vector_scores_host for one question: (rc, S float32 [V], score float32 [V])"""
    packed, x = np.ascontiguousarray(packed, np.uint64), np.ascontiguousarray(x, np.float32)
    S, sc = np.full(packed.shape[0], np.nan, np.float32), np.full(packed.shape[0], np.nan, np.float32)
    rc = _lib.lib().w2b_vector_scores_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0], D, bitlevel,
                                           x.ctypes.data_as(_lib.f32p), int(normalize), S.ctypes.data_as(_lib.f32p),
                                           sc.ctypes.data_as(_lib.f32p))
    return rc, S, sc


def query_weight(x, normalize):
    """wx of the header: nx summed in float64 column by column; 0 for a zero vector"""
    nx = np.float64(0)
    for v in np.asarray(x, np.float32):
        nx = nx + np.float64(v) * np.float64(v)
    if nx == 0:
        return np.float32(0)
    return np.float32(1.0 / np.sqrt(nx)) if normalize else np.float32(1)


def numpy_vector(M, bitlevel, x, normalize):
    """The definition on the integer matrix M [V, D], for x = n * 2^-10 with integer |n| < 2^23: every partial sum is then a
    multiple of 2^-10 below 2^26 or so, x * t is one below 2^15, and their sum is exact in float64, so float32(float64(acc) +
    float64(x) * t) is the single correctly rounded fmaf.  All rows at once, one column per step."""
    M = np.asarray(M, np.float64)
    x = np.asarray(x, np.float32)
    acc = np.zeros(M.shape[0], np.float32)
    for a in range(M.shape[1]):
        acc = (acc.astype(np.float64) + np.float64(x[a]) * M[:, a]).astype(np.float32)
    w = codes_testlib.weights(M) if bitlevel == 2 else np.float32(1.0 / np.sqrt(np.float64(M.shape[1])))
    ps = acc * query_weight(x, normalize)
    sc = ps * w
    assert ps.dtype == np.float32 and sc.dtype == np.float32
    return acc, sc


def exact_queries(rng, n, D):
    """x[a] = m * 2^-10 with integer |m| < 2^23 of every magnitude, some of them 0"""
    m = rng.integers(-2 ** 23 + 1, 2 ** 23, (n, D)) >> rng.integers(0, 23, (n, D))
    return (m.astype(np.float64) * 2.0 ** -10).astype(np.float32)


def standard_queries(rng, M, Q):
    """Q float32 questions for the integer matrix M [V, D], whose column 0 the caller has made the same in every row: Gaussian
    values times 2^randint(-20, 20) per element (any accumulation out of column order changes bits), and at the end
    [Q-5] a vector with most columns 0, [Q-4] the zero vector, [Q-3] a vector whose every score is < 0 (only column 0 set,
    against its sign), [Q-2] the negative of row 7, [Q-1] row 7 itself."""
    V, D = M.shape
    x = (rng.standard_normal((Q, D)) * np.exp2(rng.integers(-20, 21, (Q, D)))).astype(np.float32)
    x[Q - 5] = np.where(rng.random(D) < 0.9, 0, x[Q - 5])
    x[Q - 5, D // 2] = np.float32(1.5)
    x[Q - 4] = 0
    x[Q - 3] = 0
    x[Q - 3, 0] = np.float32(-2.5) * M[0, 0]                             # every S = -2.5 t^2 < 0
    x[Q - 2] = -M[7 % V].astype(np.float32)
    x[Q - 1] = M[7 % V].astype(np.float32)
    return x


def expected_lists(scores, k):
    """the lists of every question from the scores of EVERY row: (rows [Q, k], scores [Q, k])"""
    rows, out = np.empty((len(scores), k), np.int32), np.empty((len(scores), k), np.float32)
    for q, sc in enumerate(scores):
        rows[q], out[q] = answer_list(sc, sc, [], k)
    return rows, out
