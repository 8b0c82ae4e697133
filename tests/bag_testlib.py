"""Helpers of the bag-question tests (include/word2bits_eval.h, "bag questions"): the host twin, the numpy definition it is
checked against, the answer lists that scores of every row imply, and the bags every test batch contains."""
import numpy as np

from word2bits_amd import _lib
import bits_testlib
import codes_testlib

MAX_BAG = 4096


def host_bag(packed, D, bitlevel, ids):
    """w2b_bag_scores_host for one bag: (rc, J int32 [V], score float32 [V]), the bag's own rows included"""
    packed, ids = np.ascontiguousarray(packed, np.uint64), np.ascontiguousarray(ids, np.int32)
    J, sc = np.full(packed.shape[0], -77, np.int32), np.full(packed.shape[0], np.nan, np.float32)
    rc = _lib.lib().w2b_bag_scores_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0], D, bitlevel, len(ids),
                                        ids.ctypes.data_as(_lib.i32p), J.ctypes.data_as(_lib.i32p), sc.ctypes.data_as(_lib.f32p))
    return rc, J, sc


def pooled(M, ids):
    """T[a] = sum of the rows ids >= 0 of the integer matrix M, int64"""
    ids = np.asarray(ids, np.int64)
    return np.asarray(M, np.int64)[ids[ids >= 0]].sum(axis=0, dtype=np.int64)


def numpy_bag(M, bitlevel, ids):
    """the definition on the integer matrix M [V, D] (+-1, or +-1 / +-3): int64 products, the float steps one at a time"""
    M = np.asarray(M, np.int64)
    T = pooled(M, ids)
    J64 = M @ T
    assert np.abs(J64).max(initial=0) < 2 ** 31
    J = J64.astype(np.int32)
    if bitlevel == 1:
        return J, J.astype(np.float32) / np.float32(M.shape[1])
    NT = int((T * T).sum())
    wq = np.float32(1.0 / np.sqrt(np.float64(NT))) if NT else np.float32(0)
    p = J.astype(np.float32) * wq
    s = p * codes_testlib.weights(M)
    assert p.dtype == np.float32 and s.dtype == np.float32
    return J, s


def make_model(rng, bitlevel, V, D):
    """(integer matrix, packed rows): correlated rows with a block of identical ones; row 1 is the opposite of row 0"""
    if bitlevel == 1:
        M = bits_testlib.make_signs(rng, "corr", V, D)
        M[1] = -M[0]
        return M, bits_testlib.pack_signs(M)
    M = codes_testlib.make_codes(rng, "corr", V, D)
    M[1] = -M[0]
    return M, codes_testlib.pack_codes(M)


def standard_bags(rng, V):
    """empty; padding only; one id; 7 ids; 300 ids around the block of identical rows (|T| > 127: the high digit); 4096 copies
    of one row (the extremes of T); two opposite rows (T == 0 in every column)"""
    block = np.arange(V // 3, V // 3 + max(2, V // 10))
    return [np.zeros(0, np.int32), np.full(5, -1, np.int32), np.array([V - 1], np.int32),
            rng.permutation(V)[:7].astype(np.int32),
            np.concatenate([rng.choice(block, 200), rng.integers(0, V, 100)]).astype(np.int32),
            np.full(MAX_BAG, 2, np.int32), np.array([0, 1], np.int32)]


def flatten(bags):
    ids = np.concatenate([np.asarray(b, np.int32) for b in bags]).astype(np.int32)
    return ids, np.concatenate([[0], np.cumsum([len(b) for b in bags])]).astype(np.int64)


def answer_list(key, score, own, k):
    """one question's list from the values of EVERY row: `key` (J or the float score) descending, equal keys by ascending
    row, rows with key <= 0 and the rows in `own` dropped, k of them, padded with -1 / 0"""
    key = np.asarray(key).astype(np.float64)                  # exact for int32 and for float32
    ok = key > 0
    ok[np.asarray(own, np.int64)] = False
    idx = np.flatnonzero(ok)
    idx = idx[np.lexsort((idx, -key[idx]))][:k]
    rows, out = np.full(k, -1, np.int32), np.zeros(k, np.float32)
    rows[:len(idx)] = idx
    out[:len(idx)] = score[idx]
    return rows, out
