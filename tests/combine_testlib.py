"""Helpers of the tests of the signed multi-word question (include/word2bits_eval.h, w2b_eval_combine): the host twin's
scores, the answer lists they imply, and the float chain of the fp32 handles for an arbitrary query vector, generalised
from bits_testlib.oracle_chain_scores (which holds it for the three-term question)."""
import numpy as np

from word2bits_amd import _lib

MAX_TERMS = 7


def host_scores(packed, D, rows, signs):
    """w2b_bits_combine_scores_host for one question: int32 [V], the question's own rows included"""
    packed = np.ascontiguousarray(packed, np.uint64)
    rows, signs = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(signs, np.int8)
    out = np.empty(packed.shape[0], np.int32)
    _lib.check(_lib.lib().w2b_bits_combine_scores_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0], D, len(rows),
                                                       rows.ctypes.data_as(_lib.i32p), signs.ctypes.data_as(_lib.i8p),
                                                       out.ctypes.data_as(_lib.i32p)))
    return out


def numpy_scores(S, rows, signs):
    """the definition: I = ((signs[:, None] * S[rows]).sum(0) * S).sum(1) on the +-1 matrix (a sign-0 slot adds nothing)"""
    S = np.asarray(S, np.int64)
    rows, signs = np.asarray(rows, np.int64), np.asarray(signs, np.int64)
    return ((signs[:, None] * S[np.where(signs != 0, rows, 0)]).sum(0) * S).sum(1).astype(np.int32)


def ranked(score, rows, signs, k, to_float):
    """one question's answer list from the scores of EVERY row: rows other than the used slots' with score > 0, score
    descending, equal scores by ascending row, k of them; short lists end in -1 / 0"""
    s = np.array(score)
    ok = s > 0                                               # (NaN fails, like `dist > bestd`)
    ok[np.asarray(rows)[np.asarray(signs) != 0]] = False
    idx = np.flatnonzero(ok)
    idx = idx[np.lexsort((idx, -s[idx].astype(np.float64)))][:k]
    out_r, out_d = np.full(k, -1, np.int32), np.zeros(k, np.float32)
    out_r[:len(idx)] = idx
    out_d[:len(idx)] = to_float(s[idx])
    return out_r, out_d


def bits_truth(I, rows, signs, k, D):
    """[nq, k] lists from integer scores I [nq, V]; score = float32(I) / float32(D)"""
    lists = [ranked(I[q], rows[q], signs[q], k, lambda i: i.astype(np.float32) / np.float32(D)) for q in range(len(I))]
    return np.stack([x[0] for x in lists]), np.stack([x[1] for x in lists])


def float_truth(dist, rows, signs, k):
    lists = [ranked(dist[q], rows[q], signs[q], k, lambda d: d.astype(np.float32)) for q in range(len(dist))]
    return np.stack([x[0] for x in lists]), np.stack([x[1] for x in lists])


def build_vec(M, rows, signs):
    """the query vectors, float32 [nq, D]: the used slots in slot order, +-M[r0], then one float32 add or subtract each"""
    M = np.asarray(M, np.float32)
    vec = np.zeros((len(rows), M.shape[1]), np.float32)
    for q in range(len(rows)):
        first = True
        for r, s in zip(rows[q], signs[q]):
            if s == 0:
                continue
            if first:
                vec[q] = M[r] if s > 0 else -M[r]
                first = False
            else:
                vec[q] = vec[q] + M[r] if s > 0 else vec[q] - M[r]
    return vec


def chain_scores(M, vec, fma):
    """dist += vec[a] * M[c][a] for a = 0..D-1, float32 [nq, V]: bits_testlib.oracle_chain_scores for a given vec.
    fma=False: two float32 roundings per step.  fma=True: product and sum in the x87 extended format, whose 64-bit
    significand holds them exactly for float32 inputs of moderate range, rounded once to float32."""
    M, vec = np.asarray(M, np.float32), np.asarray(vec, np.float32)
    dist = np.zeros((len(vec), M.shape[0]), np.float32)
    if fma:
        assert np.finfo(np.longdouble).nmant >= 63
        Ml, vl = M.astype(np.longdouble), vec.astype(np.longdouble)
        for a in range(M.shape[1]):
            dist = (dist.astype(np.longdouble) + vl[:, a:a + 1] * Ml[None, :, a]).astype(np.float32)
    else:
        for a in range(M.shape[1]):
            dist = dist + (vec[:, a:a + 1] * M[None, :, a]).astype(np.float32)
    return dist


def random_terms(rng, V, nq, nt):
    """rows / signs [nq, nt]: mixed signs, some slots unused (sign 0, any row), some rows repeated inside a question"""
    rows = rng.integers(0, V, (nq, nt)).astype(np.int32)
    signs = rng.choice(np.array([-1, 1, 1, 0], np.int8), (nq, nt))
    signs[np.arange(nq), rng.integers(0, nt, nq)] = rng.choice(np.array([-1, 1], np.int8), nq)    # one used slot at least
    if nt >= 2:
        rep = rng.random(nq) < 0.3
        rows[rep, 1] = rows[rep, 0]
    return rows, np.ascontiguousarray(signs, np.int8)
