"""The document question (include/word2bits_eval.h, "documents"), the part that needs no GPU: the new ABI, the host twin of
the kernels against the numpy definition of docs_testlib bit for bit, every refusal with its message, the permutation property
and the fixed-point argument (every ldexp(cos, 50) seen is an integer: asserted inside docs_testlib.pair_values)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from word2bits_amd import _lib
from w2b_testlib import ROOT
from docs_testlib import flatten, host_docs, make_docs, make_model, numpy_docs, pair_values

SYMBOLS = ["w2b_eval_docs_set", "w2b_eval_docs_set_text", "w2b_eval_docs", "w2b_eval_docs_text", "w2b_eval_docs_timing",
           "w2b_docs_scores_host"]
V = 300
LENGTHS = [0, 1, 2, 63, 64, 65, 200]


def bits_of(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_eval.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\(" % name, header), name
    assert hasattr(lib, "w2b_eval_docs_count") and "w2b_eval_docs_count" in _lib.SIGNATURES
    assert re.search(r"\bint64_t\s+w2b_eval_docs_count\(", header)
    assert re.search(r"#define\s+W2B_EVAL_MAX_DOC\s+1024\b", header)


def queries_of(rng):
    qs = [rng.integers(0, V, n).astype(np.int32) for n in (1, 2, 20, 63, 64, 65, 200)]
    qs[2][[3, 7]] = -1                                            # padding ids
    qs[3][5] = qs[3][4]                                           # a repeated id
    qs += [np.full(9, -1, np.int32), np.zeros(0, np.int32)]       # all padding; no position at all
    return qs


@pytest.mark.parametrize("D", [1, 3, 64, 65, 200])
@pytest.mark.parametrize("bitlevel", [1, 2])
def test_host_twin_equals_the_numpy_definition(bitlevel, D):
    rng = np.random.default_rng(5000 + 10 * D + bitlevel)
    M, packed = make_model(rng, bitlevel, V, D)
    docs = make_docs(rng, V, 40, LENGTHS)
    assert any(len(d) and np.all(d < 0) for d in docs) and any(len(d) == 0 for d in docs)
    ids, offsets = flatten(docs)
    seen_positive = False
    for q in queries_of(rng):
        for symmetric in (0, 1):
            rc, R, sc = host_docs(packed, D, bitlevel, ids, offsets, q, symmetric)
            assert rc == 0, _lib.lib().w2b_last_error()
            wR, wsc = numpy_docs(M, bitlevel, docs, q, symmetric)
            assert np.array_equal(R, wR), (len(q), symmetric)
            assert np.array_equal(bits_of(sc), bits_of(wsc)), (len(q), symmetric)
            seen_positive |= bool(np.any(sc > 0))
            # either output alone
            _, _, s_only = host_docs(packed, D, bitlevel, ids, offsets, q, symmetric, want_dir=False)
            assert np.array_equal(bits_of(s_only), bits_of(sc))
        if not np.any(q >= 0):
            assert not R.any() and not bits_of(sc).any()          # m(Q) == 0: +0 throughout
    assert seen_positive
    empty = [d for d, doc in enumerate(docs) if not np.any(doc >= 0)]
    _, R, sc = host_docs(packed, D, bitlevel, ids, offsets, np.array([0, 1, 2], np.int32), 1)
    assert not R[:, empty].any() and not bits_of(sc[empty]).any()     # m(D) == 0: +0


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_permuting_positions_changes_no_bit(bitlevel):
    rng = np.random.default_rng(77 + bitlevel)
    D = 65
    M, packed = make_model(rng, bitlevel, V, D)
    docs = make_docs(rng, V, 20, [1, 2, 63, 65, 200])
    q = rng.integers(0, V, 30).astype(np.int32)
    q[4] = -1
    ids, offsets = flatten(docs)
    _, R, sc = host_docs(packed, D, bitlevel, ids, offsets, q, 1)
    ids2, _ = flatten([rng.permutation(d) for d in docs])
    _, R2, sc2 = host_docs(packed, D, bitlevel, ids2, offsets, rng.permutation(q), 1)
    assert np.array_equal(R, R2) and np.array_equal(bits_of(sc), bits_of(sc2))


def test_fixed_point_image_is_integral_and_never_minus_zero():
    """pair_values asserts it for every value it converts; here on rows built to be orthogonal (J == 0: cos must be +0) and
    opposite (cos near -1), at sizes whose weights are not powers of two -- and the twin, asked with one-id texts, must return
    exactly these integers as A of both directions, and the score A / 2^50 = cos itself, +0 where J == 0"""
    import codes_testlib
    for D in (2, 7, 200, 1000):
        T = np.ones((6, D), np.int8)
        T[1] = -1
        T[2, ::2] = -1                                           # J(0, 2) == 0 for even D
        T[3] = 3
        T[4, :D // 2] = 3
        T[5, 1::2] = -3
        F = pair_values(T, 2, np.arange(6))
        assert F.dtype == np.int64 and (D % 2 or F[0, 2] == 0)
        assert np.abs(F).max() <= (1 << 50) + (1 << 28)           # |cos| <= 1 + a few ulp
        packed = codes_testlib.pack_codes(T)
        for x in range(6):
            rc, A, sc = host_docs(packed, D, 2, np.arange(6), np.arange(7), np.array([x], np.int32), 1)
            assert rc == 0
            assert np.array_equal(A[0], F[x]) and np.array_equal(A[1], F[x]), (D, x)
            cos = np.ldexp(F[x].astype(np.float64), -50).astype(np.float32)        # exact: F is a float32 scaled by 2^50
            assert np.array_equal(bits_of(sc), bits_of(cos)), (D, x)
            assert not np.any(np.signbit(sc) & (sc == 0))
        if D % 2 == 0:
            assert bits_of(host_docs(packed, D, 2, np.arange(6), np.arange(7), np.array([0], np.int32), 0)[2])[2] == 0


def test_refusals_and_untouched_outputs():
    rng = np.random.default_rng(3)
    D = 65
    M, packed = make_model(rng, 1, V, D)
    L = _lib.lib()
    p = packed.ctypes.data_as(_lib.u64p)
    ids = np.array([1, 2, -1, 3], np.int32)
    off = np.array([0, 2, 4], np.int64)
    q = np.array([5, 6], np.int32)
    R, sc = np.full((2, 2), -77, np.int64), np.full(2, 7.0, np.float32)

    def call(words=V, dim=D, bitlevel=1, ids=ids, n_docs=2, off=off, q=q, symmetric=1, n_ids=None):
        return L.w2b_docs_scores_host(p, words, dim, bitlevel, len(ids) if n_ids is None else n_ids, ids.ctypes.data_as(_lib.i32p),
                                      n_docs, off.ctypes.data_as(_lib.i64p), len(q), q.ctypes.data_as(_lib.i32p), symmetric,
                                      R.ctypes.data_as(_lib.i64p), sc.ctypes.data_as(_lib.f32p))

    def refused(msg, **kw):
        assert call(**kw) == _lib.W2B_EINVAL
        assert msg in L.w2b_last_error(), L.w2b_last_error()

    refused(b"symmetric must be 0 or 1", symmetric=2)
    refused(b"symmetric must be 0 or 1", symmetric=-1)
    refused(b"a query holds at most 1024 positions", q=np.zeros(1025, np.int32))
    refused(b"offsets must start at 0", off=np.array([1, 2, 4], np.int64))
    refused(b"offsets must start at 0", off=np.array([0, 2, 3], np.int64))
    refused(b"offsets must not decrease", off=np.array([0, 5, 4], np.int64))
    refused(b"offsets must not decrease", off=np.array([0, -1, 4], np.int64))
    long_ids = np.zeros(1025, np.int32)
    refused(b"a document holds at most 1024 positions", ids=long_ids, n_docs=1, off=np.array([0, 1025], np.int64))
    refused(b"at most 0x7FFFFF00 documents", n_docs=0x7FFFFF01)              # (refused before the offsets are read)
    refused(b"at most 0x7FFFFF00 documents", n_docs=0x7FFFFF01, bitlevel=3)
    refused(b"bitlevel must be 1 or 2", bitlevel=3)
    refused(b"size must be below 2^21", dim=1 << 21)
    refused(b"document id out of range", ids=np.array([1, 2, V, 3], np.int32))
    refused(b"query id out of range", q=np.array([5, V], np.int32))
    # the order: what needs no table first
    refused(b"symmetric must be 0 or 1", symmetric=2, bitlevel=3, ids=np.array([1, 2, V, 3], np.int32))
    refused(b"offsets must not decrease", off=np.array([0, 5, 4], np.int64), bitlevel=3)
    assert np.all(R == -77) and np.all(sc == 7.0)                 # refused: nothing written
    assert call() == _lib.W2B_OK and not np.any(R == -77)
    # 1024 positions, padding included, are allowed; an id < 0 is never out of range
    ok_ids = np.full(1024, -5, np.int32)
    R, sc = np.full((2, 1), -77, np.int64), np.full(1, 7.0, np.float32)
    assert call(ids=ok_ids, n_docs=1, off=np.array([0, 1024], np.int64), q=np.full(1024, -1, np.int32)) == _lib.W2B_OK
    assert not R.any() and not bits_of(sc).any()


def test_device_entry_points_validate_before_they_need_a_handle():
    """a NULL handle with a bad k is W2B_EINVAL for the k; the order is that of w2b_eval_bag"""
    L = _lib.lib()
    ids = np.array([1, 2], np.int32)
    off = np.array([0, 2], np.int64)
    best, bestd = np.full(4, -9, np.int32), np.full(4, 7.0, np.float32)
    ip, op, bp, dp = (a.ctypes.data_as(t) for a, t in ((ids, _lib.i32p), (off, _lib.i64p), (best, _lib.i32p), (bestd, _lib.f32p)))

    def docs(k=4, symmetric=1, op=op, n_ids=2):
        return L.w2b_eval_docs(None, n_ids, ip, 1, op, symmetric, k, bp, dp, None)

    for k in (0, 65, -1):
        assert docs(k=k) == _lib.W2B_EINVAL and b"k must be 1..64" in L.w2b_last_error()
    assert docs(symmetric=2) == _lib.W2B_EINVAL and b"symmetric must be 0 or 1" in L.w2b_last_error()
    bad = np.array([0, 3], np.int64)
    assert docs(op=bad.ctypes.data_as(_lib.i64p)) == _lib.W2B_EINVAL and b"offsets must start at 0" in L.w2b_last_error()
    long_off = np.array([0, 1025], np.int64)
    long_ids = np.zeros(1025, np.int32)
    assert L.w2b_eval_docs(None, 1025, long_ids.ctypes.data_as(_lib.i32p), 1, long_off.ctypes.data_as(_lib.i64p), 1, 4, bp, dp,
                           None) == _lib.W2B_EINVAL and b"a query holds at most 1024 positions" in L.w2b_last_error()
    assert docs() == _lib.W2B_EINVAL and b"null handle" in L.w2b_last_error()
    # no query: W2B_OK once the checks that need no handle have passed -- but not before them
    zero = np.zeros(1, np.int64)
    assert L.w2b_eval_docs(None, 0, ip, 0, zero.ctypes.data_as(_lib.i64p), 1, 4, bp, dp, None) == _lib.W2B_OK
    assert L.w2b_eval_docs(None, 0, ip, 0, zero.ctypes.data_as(_lib.i64p), 1, 0, bp, dp, None) == _lib.W2B_EINVAL
    assert L.w2b_eval_docs(None, 2, ip, 0, zero.ctypes.data_as(_lib.i64p), 1, 4, bp, dp, None) == _lib.W2B_EINVAL
    assert np.all(best == -9) and np.all(bestd == 7.0)
    assert L.w2b_eval_docs_set(None, 1025, long_ids.ctypes.data_as(_lib.i32p), 1, long_off.ctypes.data_as(_lib.i64p)) == _lib.W2B_EINVAL
    assert b"a document holds at most 1024 positions" in L.w2b_last_error()
    assert L.w2b_eval_docs_set(None, 2, ip, 1, op) == _lib.W2B_EINVAL and b"null handle" in L.w2b_last_error()
    assert L.w2b_eval_docs_set(None, 2, ip, 0x7FFFFF01, op) == _lib.W2B_EINVAL
    assert b"at most 0x7FFFFF00 documents" in L.w2b_last_error()
    out, n = C.c_void_p(), C.c_int64()
    assert L.w2b_eval_docs_text(None, b"a", 1, 1, 0, C.byref(out), C.byref(n)) == _lib.W2B_EINVAL
    assert b"k must be 1..64" in L.w2b_last_error()
    assert L.w2b_eval_docs_count(None) == 0
