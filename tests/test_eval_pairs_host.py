"""Pair similarity (include/word2bits_eval.h, "pair similarity"), the part that needs no GPU: the new ABI, the host twin of the
kernels against the numpy definition of pairs_testlib bit for bit (parts as integers, scores as uint32 patterns), the two
consequences the header states, every refusal with its message, and the rank correlations against a numpy restatement (and
scipy, where it is installed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT
from pairs_testlib import (MAX_BAG, ONE, flatten_pairs, host_pairs, make_model, numpy_correlations, numpy_pairs,
                           standard_pairs)

SYMBOLS = ["w2b_eval_pairs", "w2b_eval_pairs_text", "w2b_pairs_host", "w2b_rank_correlation"]
V = 300
LENGTHS = [0, 1, 2, 64, 65, 4096]


def bits_of(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_eval.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\(" % name, header), name
    assert callable(w2b.rank_correlation) and hasattr(w2b.Evaluator, "pairs") and hasattr(w2b.Evaluator, "pairs_text")
    assert hasattr(w2b.Evaluator, "similarity")


@pytest.mark.parametrize("D", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("bitlevel", [1, 2])
def test_host_twin_equals_the_numpy_definition(bitlevel, D):
    rng = np.random.default_rng(7000 + 10 * D + bitlevel)
    M, packed = make_model(rng, bitlevel, V, D)
    pairs, named = standard_pairs(rng, V, LENGTHS)
    assert any(len(a) == MAX_BAG and len(b) == MAX_BAG for a, b in pairs)
    ids, offsets = flatten_pairs(pairs)
    rc, score, parts = host_pairs(packed, D, bitlevel, ids, offsets)
    assert rc == 0, _lib.lib().w2b_last_error()
    want_parts, want_score = numpy_pairs(M, pairs)
    assert np.array_equal(parts, want_parts), np.argwhere(parts != want_parts)[:10]
    assert np.array_equal(bits_of(score), bits_of(want_score))
    # either output alone
    _, s_only, _ = host_pairs(packed, D, bitlevel, ids, offsets, want_parts=False)
    _, _, p_only = host_pairs(packed, D, bitlevel, ids, offsets, want_score=False)
    assert np.array_equal(bits_of(s_only), bits_of(score)) and np.array_equal(p_only, parts)
    # identical bags score exactly 1, in any order of their ids
    for name in ("identical", "identical_permuted", "identical_long", "one_word_same"):
        assert bits_of(score[named[name]]) == 0x3F800000 == bits_of(ONE), name
    # empty pairs: +0, and the side that is empty has N == 0
    for name in ("empty_no_ids", "empty_both", "empty_padding", "empty_cancels", "one_padding_word"):
        p = named[name]
        assert bits_of(score[p]) == 0 and (parts[p, 1] == 0 or parts[p, 2] == 0) and parts[p, 0] == 0, name
    assert parts[named["empty_cancels"], 2] > 0
    # the opposite row: exactly -1
    assert score[named["one_word_opposite"]] == -1.0
    # padding contributes nothing, a repeated row adds
    assert np.array_equal(parts[named["padding"]], numpy_pairs(M, [([5, 9, 9], [200, 7])])[0][0])
    assert np.array_equal(parts[named["one_word_and_padding"]], parts[named["one_word"]])
    # the trap of the last word: N of a one-word bag counts the `size` columns alone
    p = named["one_word"]
    assert parts[p, 1] == (D if bitlevel == 1 else int((M[V - 1].astype(np.int64) ** 2).sum()))
    assert np.any(score > 0) and np.any(score < 0)


@pytest.mark.parametrize("D", [1, 63, 65, 200])
def test_bits_one_word_pairs_score_like_the_neighbour_scan(D):
    """N_A = N_B = size, and the score is float32(J) / float32(size): the bits neighbours' and bags' expression"""
    rng = np.random.default_rng(D)
    M, packed = make_model(rng, 1, V, D)
    rows = rng.integers(0, V, (400, 2)).astype(np.int32)
    rows[:5, 1] = rows[:5, 0]
    rows[5] = 0, 1
    rc, score, parts = host_pairs(packed, D, 1, rows.ravel(), np.arange(801))
    assert rc == 0
    assert np.all(parts[:, 1] == D) and np.all(parts[:, 2] == D)
    J = (M[rows[:, 0]].astype(np.int64) * M[rows[:, 1]]).sum(axis=1)
    assert np.array_equal(parts[:, 0], J)
    assert np.array_equal(bits_of(score), bits_of(J.astype(np.float32) / np.float32(D)))


def test_refusals_and_untouched_outputs():
    rng = np.random.default_rng(3)
    D = 65
    M, packed = make_model(rng, 1, V, D)
    L = _lib.lib()
    ids = np.array([1, 2, -1, 3], np.int32)
    off = np.array([0, 2, 4], np.int64)

    def refused(msg, ids=ids, off=off, dim=D, bitlevel=1, **kw):
        rc, score, parts = host_pairs(packed, dim, bitlevel, ids, off, **kw)
        assert rc == _lib.W2B_EINVAL
        assert msg in L.w2b_last_error(), L.w2b_last_error()
        assert np.all(np.isnan(score)) and np.all(parts == -77)           # refused: nothing written

    refused(b"offsets must start at 0", off=np.array([1, 2, 4], np.int64))
    refused(b"offsets must start at 0", off=np.array([0, 2, 3], np.int64))
    refused(b"offsets must not decrease", off=np.array([0, 5, 4], np.int64))
    refused(b"offsets must not decrease", off=np.array([0, -1, 4], np.int64))
    big = np.zeros(MAX_BAG + 1, np.int32)
    refused(b"a bag holds at most 4096 ids", ids=big, off=np.array([0, MAX_BAG + 1, MAX_BAG + 1], np.int64))
    refused(b"a bag holds at most 4096 ids", ids=big, off=np.array([0, 0, MAX_BAG + 1], np.int64))
    refused(b"bitlevel must be 1 or 2", bitlevel=3)
    refused(b"bitlevel must be 1 or 2", bitlevel=0)
    refused(b"size must be at most 2^24", dim=(1 << 24) + 1)
    refused(b"pair 0: id out of range", ids=np.array([1, 2, V, 3], np.int32))
    two = np.array([0, 1, 2, 3, 4], np.int64)
    refused(b"pair 1: id out of range", ids=np.array([1, 2, 3, V], np.int32), off=two)
    refused(b"bad argument", want_score=False, want_parts=False)
    # the order: what needs no table first
    refused(b"offsets must not decrease", off=np.array([0, 5, 4], np.int64), bitlevel=3, ids=np.array([1, 2, V, 3], np.int32))
    refused(b"bitlevel must be 1 or 2", bitlevel=3, ids=np.array([1, 2, V, 3], np.int32))
    rc, score, parts = host_pairs(packed, D, 1, ids, off)
    assert rc == _lib.W2B_OK and not np.any(np.isnan(score)) and not np.any(parts == -77)
    # 4096 ids, padding included, are allowed; an id < 0 is never out of range; no pair at all is fine
    ok = np.full(2 * MAX_BAG, -5, np.int32)
    rc, score, parts = host_pairs(packed, D, 1, ok, np.array([0, MAX_BAG, 2 * MAX_BAG], np.int64))
    assert rc == _lib.W2B_OK and not parts.any() and not bits_of(score).any()
    assert host_pairs(packed, D, 1, np.zeros(0, np.int32), np.zeros(1, np.int64))[0] == _lib.W2B_OK
    assert host_pairs(packed, D, 1, np.zeros(2, np.int32), np.zeros(1, np.int64))[0] == _lib.W2B_EINVAL


def test_device_entry_points_validate_before_they_need_a_handle():
    """a NULL handle with bad offsets is W2B_EINVAL for the offsets; the order is that of w2b_eval_bag"""
    L = _lib.lib()
    ids = np.array([1, 2], np.int32)
    score, parts = np.full(1, 7.0, np.float32), np.full(3, -9, np.int64)
    ip, sp, pp = ids.ctypes.data_as(_lib.i32p), score.ctypes.data_as(_lib.f32p), parts.ctypes.data_as(_lib.i64p)

    def pairs(off, n_ids=2, n=1, sp=sp):
        off = np.asarray(off, np.int64)
        return L.w2b_eval_pairs(None, n_ids, ip, n, off.ctypes.data_as(_lib.i64p), sp, pp)

    assert pairs([0, 1, 3]) == _lib.W2B_EINVAL and b"offsets must start at 0" in L.w2b_last_error()
    assert pairs([0, 3, 2]) == _lib.W2B_EINVAL and b"offsets must not decrease" in L.w2b_last_error()
    big = np.zeros(MAX_BAG + 1, np.int32)
    off = np.array([0, MAX_BAG + 1, MAX_BAG + 1], np.int64)
    assert L.w2b_eval_pairs(None, MAX_BAG + 1, big.ctypes.data_as(_lib.i32p), 1, off.ctypes.data_as(_lib.i64p), sp,
                            pp) == _lib.W2B_EINVAL and b"a bag holds at most 4096 ids" in L.w2b_last_error()
    assert pairs([0, 1, 2], n=-1) == _lib.W2B_EINVAL and b"bad argument" in L.w2b_last_error()
    assert pairs([0, 1, 2], sp=None) == _lib.W2B_EINVAL and b"bad argument" in L.w2b_last_error()
    assert pairs([0, 1, 2]) == _lib.W2B_EINVAL and b"null handle" in L.w2b_last_error()
    assert pairs([0], n_ids=0, n=0) == _lib.W2B_EINVAL and b"null handle" in L.w2b_last_error()
    assert pairs([0], n_ids=2, n=0) == _lib.W2B_EINVAL and b"offsets must start at 0" in L.w2b_last_error()
    assert np.all(score == 7.0) and np.all(parts == -9)
    out, n = C.c_void_p(), C.c_int64()
    assert L.w2b_eval_pairs_text(None, b"a\tb\t1\n", 6, 1, C.byref(out), C.byref(n)) == _lib.W2B_EINVAL
    assert b"null handle" in L.w2b_last_error()
    assert L.w2b_eval_pairs_text(None, b"a", 1, 1, None, C.byref(n)) == _lib.W2B_EINVAL and b"bad argument" in L.w2b_last_error()


def test_rank_correlation_equals_the_numpy_restatement():
    """both sides are double sums in different orders: their rounding error is around 1e-13, the margin 1e-9 is generous and
    still far below any real difference"""
    rng = np.random.default_rng(11)
    seen_ties = False
    for n in (2, 3, 10, 353, 999, 10000):
        for kind in ("normal", "ties", "anti", "scores"):
            x = rng.normal(size=n)
            y = 0.6 * x + rng.normal(size=n)
            if kind == "ties":                                   # human ratings on a coarse scale, cosines of few values
                x, y = np.round(x * 2) / 2, np.round(y * 3) / 3
                seen_ties |= len(np.unique(x)) < n
            elif kind == "anti":
                y = -x
            elif kind == "scores":
                x, y = rng.integers(0, 11, n).astype(np.float64), (rng.integers(-200, 201, n) / 200).astype(np.float32)
            r, rho = w2b.rank_correlation(x, y)
            wr, wrho = numpy_correlations(x, y)
            if np.isnan(wr):
                assert np.isnan(r) and np.isnan(rho), (n, kind)
                continue
            assert abs(r - wr) <= 1e-9 and abs(rho - wrho) <= 1e-9, (n, kind, r, wr, rho, wrho)
            if kind == "anti":
                assert abs(r + 1) <= 1e-9 and abs(rho + 1) <= 1e-9
    assert seen_ties
    # a monotone map changes Pearson and leaves Spearman at exactly 1
    x = np.arange(1.0, 50.0)
    r, rho = w2b.rank_correlation(x, np.exp(x / 5))
    assert r < 0.95 and rho == 1.0
    # average ranks by hand: x = 1 2 2 3 -> ranks 1 2.5 2.5 4
    r, rho = w2b.rank_correlation([1, 2, 2, 3], [1, 2, 3, 4])
    want = numpy_correlations([1, 2.5, 2.5, 4], [1, 2, 3, 4])[0]
    assert abs(rho - want) <= 1e-12


def test_rank_correlation_equals_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(12)
    for n in (2, 17, 353, 10000):
        x = np.round(rng.normal(size=n) * 4) / 4
        y = 0.5 * x + rng.normal(size=n)
        y[: n // 3] = np.round(y[: n // 3])
        r, rho = w2b.rank_correlation(x, y)
        if len(np.unique(x)) < 2 or len(np.unique(y)) < 2:
            continue
        assert abs(r - stats.pearsonr(x, y)[0]) <= 1e-9
        assert abs(rho - stats.spearmanr(x, y)[0]) <= 1e-9


def test_rank_correlation_is_nan_without_variance():
    for x, y in (([], []), ([1.0], [2.0]), ([1, 1, 1], [1, 2, 3]), ([1, 2, 3], [5, 5, 5]), ([1, 2, np.nan], [1, 2, 3])):
        r, rho = w2b.rank_correlation(x, y)
        assert np.isnan(r) and np.isnan(rho), (x, y)
    r, rho = w2b.rank_correlation([1, 2], [2, 1])
    assert r == -1.0 and rho == -1.0
    L = _lib.lib()
    assert L.w2b_rank_correlation(-1, None, None, None, None) == _lib.W2B_EINVAL
    assert L.w2b_rank_correlation(2, None, None, None, None) == _lib.W2B_EINVAL and b"bad argument" in L.w2b_last_error()
    assert L.w2b_rank_correlation(0, None, None, None, None) == _lib.W2B_OK
    with pytest.raises(ValueError):
        w2b.rank_correlation([1, 2], [1])
