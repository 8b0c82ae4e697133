"""Helpers of the codes-mode evaluator tests: a numpy implementation of the semantics in include/word2bits_eval.h
("codes mode") -- t matrices from packed words, exact integer products through a float32 sgemm (|J| <= 9 D < 2^24), the
per-row weights, the float32 score sequence, the list order -- plus 2-bit models to test on and the packed model file."""
import numpy as np

import word2bits_amd as w2b


def make_codes(rng, kind, V, D):
    """[V, D] int8 in {-3, -1, +1, +3}.  "random": independent values.  "corr": noisy copies of a few prototypes and a
    block of identical rows (ties at the top of every list that reaches it)."""
    T = ((rng.integers(0, 2, (V, D)) * 2 - 1) * (rng.integers(0, 2, (V, D)) * 2 + 1)).astype(np.int8)
    if kind == "random" or V < 8:
        return T
    proto = T[:4].copy()
    C = proto[rng.integers(0, 4, V)]
    noise = rng.random((V, D)) < rng.choice([0.02, 0.1, 0.3], (V, 1))
    C = np.where(noise, T, C).astype(np.int8)
    n = max(2, V // 10)
    C[V // 3:V // 3 + n] = C[V // 3]
    return C


def values_of(T):
    """the bitlevel-2 float values of a t matrix"""
    return (np.asarray(T, np.float32) * np.float32(0.25)).astype(np.float32)


def pack_codes(T):
    """uint64 [V, 2 * ceil(D / 64)] through w2b_pack_quantized: the file's layout"""
    return w2b.pack_quantized(values_of(T), 2)


def codes_of_packed(packed, D):
    """the t matrix that packed words stand for: per 64 columns a sign word, then a magnitude word"""
    packed = np.ascontiguousarray(packed, "<u8")
    V = packed.shape[0]
    bits = np.unpackbits(packed.view(np.uint8).reshape(V, -1, 2, 8), axis=3, bitorder="little")   # [V, nb, 2, 64]
    sign = bits[:, :, 0, :].reshape(V, -1)[:, :D].astype(np.int8)
    mag = bits[:, :, 1, :].reshape(V, -1)[:, :D].astype(np.int8)
    return ((1 - 2 * sign) * (1 + 2 * mag)).astype(np.int8)


def write_packed_file(path, names, packed, D):
    """the .w2bp format of include/word2bits_corpus.h, bitlevel 2"""
    packed = np.ascontiguousarray(packed, "<u8")
    with open(path, "wb") as f:
        f.write(b"W2BP1 %d %d 2\n" % (packed.shape[0], D))
        for n in names:
            f.write(n + b"\n")
        f.write(packed.tobytes())
    return path


def weights(T):
    """w(r) = float32(1 / sqrt(float64(D + 8 n3(r))))"""
    T = np.asarray(T)
    n3 = (np.abs(T) == 3).sum(1)
    return (1.0 / np.sqrt((T.shape[1] + 8 * n3).astype(np.float64))).astype(np.float32)


def int_products(T, rows):
    """J[q, c] = sum_a T[rows[q]][a] * T[c][a], int32 [nq, V]; float32 holds every partial sum exactly"""
    T = np.asarray(T)
    X = T[np.asarray(rows, np.int64)].astype(np.float32)
    out = np.empty((X.shape[0], T.shape[0]), np.int32)
    for r0 in range(0, T.shape[0], 65536):
        out[:, r0:r0 + 65536] = np.rint(X @ T[r0:r0 + 65536].astype(np.float32).T).astype(np.int32)
    return out


def scores(T, b1, b2, b3):
    """float32 [nq, V]: ((J2 w(b2) - J1 w(b1)) + J3 w(b3)) w(c), every operation a float32 operation of its own"""
    b1, b2, b3 = (np.asarray(x, np.int64) for x in (b1, b2, b3))
    w = weights(T)
    p1 = int_products(T, b1).astype(np.float32) * w[b1][:, None]
    p2 = int_products(T, b2).astype(np.float32) * w[b2][:, None]
    p3 = int_products(T, b3).astype(np.float32) * w[b3][:, None]
    s = ((p2 - p1) + p3) * w[None, :]
    assert s.dtype == np.float32
    return s


def truth_from_scores(S, b1, b2, b3, k):
    """the answer lists: rows other than b1, b2, b3 with score > 0, score descending, equal scores by ascending row, k of
    them, short lists ending in -1 / 0"""
    nq = S.shape[0]
    rows, out = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float32)
    for q in range(nq):
        s = S[q].copy()
        s[[b1[q], b2[q], b3[q]]] = 0
        idx = np.flatnonzero(s > 0)
        idx = idx[np.lexsort((idx, -s[idx].astype(np.float64)))][:k]
        rows[q, :len(idx)] = idx
        out[q, :len(idx)] = s[idx]
    return rows, out


def truth_topk(T, b1, b2, b3, k):
    b1, b2, b3 = (np.asarray(x, np.int64) for x in (b1, b2, b3))
    return truth_from_scores(scores(T, b1, b2, b3), b1, b2, b3, k)


def truth_top1(T, b1, b2, b3):
    r, d = truth_topk(T, b1, b2, b3, 1)
    return r[:, 0], d[:, 0]


def lead_over_runner_up(S, b1, b2, b3):
    """per question: best allowed score minus the second best allowed score (scores <= 0 count as 0), float64"""
    out = np.empty(S.shape[0])
    for q in range(S.shape[0]):
        s = np.maximum(S[q].astype(np.float64), 0)
        s[[b1[q], b2[q], b3[q]]] = 0
        top = np.partition(s, -2)[-2:]
        out[q] = top[1] - top[0]
    return out


def float_bound(D):
    """|fp32 chain score - codes score| <= (3 D + 38) 2^-24, to first order in u = 2^-24.  Both are compared with the
    exact S = (J2/sqrt(N2) - J1/sqrt(N1) + J3/sqrt(N3)) / sqrt(Nc), a combination of dot products of unit vectors.
    fp32 path: the squared length N/16 is exact in float (9 D < 2^24), so a normalised value is t/sqrt(N) within 2 u
    (sqrtf, division); vec = (M2 - M1) + M3 adds two roundings: |dvec[a]| <= 4 u (|M1[a]| + |M2[a]| + |M3[a]|), which
    against the unit row c is <= 12 u (Cauchy-Schwarz), and row c's own error against |vec|_2 <= 3 is <= 6 u; each of the D
    chain steps rounds a partial sum of magnitude <= sum |vec[a] M[c][a]| <= 3: 3 D u, and the unfused build rounds the
    products too: 3 u.  Together (3 D + 21) u.  Codes path: w within u, so p_i within 2 u |J_i| / sqrt(N_i) (6 u after the
    scale by w(c), each term being <= 1), the subtraction rounds a value <= 2 and the addition one <= 3 (5 u), w(c) and
    the last product 2 u of a value <= 3 (6 u): 17 u."""
    return (3 * D + 38) * 2.0 ** -24


class TruthModel:
    """what oracle/eval_oracle.py's transcript() asks of a model, with top1 answered by the numpy truth; names and lookup
    are those of `om`, an EvalModel of the float file of the same model loaded with bitlevel 2"""

    def __init__(self, om, T):
        self.words, self.size, self.names, self.first = om.words, om.size, om.names, om.first
        self.T = T

    def lookup(self, st):
        return self.first.get(st, self.words)

    def top1(self, b1, b2, b3):
        return truth_top1(self.T, np.asarray(b1, np.int64), np.asarray(b2, np.int64), np.asarray(b3, np.int64))
