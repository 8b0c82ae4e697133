"""Helpers of the word-class tests (include/word2bits_eval.h, "word classes"): the host twin, an independent numpy restatement
of the k-means loop it is checked against, planted models, purity, and the text form."""
import numpy as np

from word2bits_amd import _lib
import bits_testlib
import codes_testlib
from bag_testlib import make_model   # noqa: F401  (re-exported for the tests)

MAX_CLASSES = 16384
MAX_WORDS = 5592405
SENTINEL_I, SENTINEL_F = -77, np.float32(7.5)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def outputs(V, D, K):
    """the six outputs of one call, filled with sentinels: cls, score, T, counts, iters_run [1], moved [1]"""
    K = max(int(K), 1)
    return (np.full(V, SENTINEL_I, np.int32), np.full(V, SENTINEL_F, np.float32), np.full((K, D), SENTINEL_I, np.int32),
            np.full(K, SENTINEL_I, np.int64), np.full(1, SENTINEL_I, np.int32), np.full(1, SENTINEL_I, np.int64))


def untouched(out):
    return (np.all(out[0] == SENTINEL_I) and np.all(out[1] == SENTINEL_F) and np.all(out[2] == SENTINEL_I) and
            np.all(out[3] == SENTINEL_I) and out[4][0] == SENTINEL_I and out[5][0] == SENTINEL_I)


def host_classes_raw(packed, D, bitlevel, K, iters, init, out, words=None):
    """w2b_classes_host into `out` (see outputs): (rc, last error)"""
    packed = None if packed is None else np.ascontiguousarray(packed, np.uint64)
    init = None if init is None else np.ascontiguousarray(init, np.int32)
    V = packed.shape[0] if words is None else words
    L = _lib.lib()
    rc = L.w2b_classes_host(_p(packed, _lib.u64p), V, D, bitlevel, K, iters, _p(init, _lib.i32p), _p(out[0], _lib.i32p),
                            _p(out[1], _lib.f32p), _p(out[2], _lib.i32p), _p(out[3], _lib.i64p), _p(out[4], _lib.i32p),
                            _p(out[5], _lib.i64p))
    return rc, L.w2b_last_error()


def host_classes(packed, D, bitlevel, K, iters, init=None):
    """the C twin: (cls, score, T, counts, iters_run, moved)"""
    out = outputs(packed.shape[0], D, K)
    rc, why = host_classes_raw(packed, D, bitlevel, K, iters, init, out)
    assert rc == 0, why
    return out[0], out[1], out[2], out[3], int(out[4][0]), int(out[5][0])


def class_sums(M, cl, K):
    """T [K, D] int64 and counts [K] of the class array cl: np.add.at on the integer matrix"""
    T = np.zeros((K, M.shape[1]), np.int64)
    for i in range(0, len(M), 50000):                          # (slices widened to the sum's type: ufunc.at is slow when it casts)
        np.add.at(T, np.asarray(cl[i:i + 50000], np.int64), M[i:i + 50000].astype(np.int64))
    return T, np.bincount(cl, minlength=K).astype(np.int64)


def numpy_classes(M, K, iters, init=None, reverse=False):
    """The loop of the header on the integer matrix M [V, D], independent of the twin.  The chain goes column by column for
    all (row, class) pairs at once as float32(float64(acc) + float64(T) * t): acc is an integer-valued float32, T * t an
    integer below 2^27, their sum an integer far below 2^53 and so exact in float64 -- the conversion is then the single
    correctly rounded step of fmaf (the argument of vectors_testlib.numpy_vector).  reverse=True walks the columns from the
    last to the first: NOT the definition, for tests that show the order matters.  Returns what host_classes returns."""
    M = np.asarray(M, np.int8)
    V, D = M.shape
    Mt = np.ascontiguousarray(M.T)                                    # [D, V]
    cl = (np.arange(V) % K).astype(np.int32) if init is None else np.asarray(init, np.int32).copy()
    score, it, moved = np.zeros(V, np.float32), 0, 0
    cols = range(D - 1, -1, -1) if reverse else range(D)
    while it < iters:
        T, _ = class_sums(M, cl, K)
        N = (T * T).sum(axis=1)
        live = np.flatnonzero(N > 0)
        wq = (1.0 / np.sqrt(N[live].astype(np.float64))).astype(np.float32)
        if len(live):
            Tl = T[live].astype(np.float64)                             # dead classes never compete: leave them out
            acc = np.zeros((V, len(live)), np.float32)
            for a in cols:
                acc = (acc.astype(np.float64) + Mt[a].astype(np.float64)[:, None] * Tl[:, a][None, :]).astype(np.float32)
            d = acc * wq[None, :]
            assert d.dtype == np.float32
            j = np.argmax(d, axis=1)                                    # the first of equal maxima: the lowest class
            new, score = live[j].astype(np.int32), d[np.arange(V), j]
        else:
            new, score = np.zeros(V, np.int32), np.zeros(V, np.float32)
        moved = int((new != cl).sum())
        cl = new
        it += 1
        if moved == 0:
            break
    T, counts = class_sums(M, cl, K)
    return cl, score, T.astype(np.int32), counts, it, moved


def same_result(a, b):
    """every output equal, scores by bit pattern"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and
            np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4] and a[5] == b[5])


def pack(M, bitlevel):
    """the packed rows of an integer matrix, in slices (a 200 000-row model is not expanded to floats at once)"""
    f = bits_testlib.pack_signs if bitlevel == 1 else codes_testlib.pack_codes
    return np.concatenate([f(M[i:i + 20000]) for i in range(0, len(M), 20000)])


def planted(rng, bitlevel, V, D, P, flip):
    """(M, packed, labels): V rows drawn from P prototypes, the sign of every value flipped with probability `flip`"""
    proto = (rng.integers(0, 2, (P, D)) * 2 - 1).astype(np.int8)
    if bitlevel == 2:
        proto = (proto * (rng.integers(0, 2, (P, D)) * 2 + 1)).astype(np.int8)
    labels = rng.integers(0, P, V)
    M = np.where(rng.random((V, D)) < flip, -proto[labels], proto[labels]).astype(np.int8)
    return M, pack(M, bitlevel), labels


def purity(cls, labels, K):
    """the share of rows whose label is the most frequent one of their class"""
    hit = 0
    for k in range(K):
        l = labels[cls == k]
        if len(l):
            hit += np.bincount(l).max()
    return hit / len(cls)


def class_lines(names, cls):
    """word2vec's -classes format: the upper-cased word, a space, the class"""
    return b"".join(n.upper() + b" %d\n" % c for n, c in zip(names, cls))
