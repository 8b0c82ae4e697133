"""Helpers of the bits-mode evaluator tests: a numpy implementation of the semantics in include/word2bits_eval.h
("bits mode") -- integer scores, list order, float scores -- sign matrices to test on, the packed model file, and the
float oracle's score chains in numpy (checked against the pinned oracle where they are used)."""
import numpy as np

import word2bits_amd as w2b

THIRD = np.float32(1) / np.float32(3)            # the magnitude of a bitlevel-1 value


def make_signs(rng, kind, V, D):
    """[V, D] int8 in {+1, -1}.  "random": independent signs.  "corr": noisy copies of a few prototypes, and a block of
    identical rows (massive ties at the top of every list that reaches it)."""
    if kind == "random" or V < 8:
        return (rng.integers(0, 2, (V, D)) * 2 - 1).astype(np.int8)
    proto = (rng.integers(0, 2, (4, D)) * 2 - 1).astype(np.int8)
    S = proto[rng.integers(0, 4, V)]
    flip = rng.random((V, D)) < rng.choice([0.02, 0.1, 0.3], (V, 1))
    S = np.where(flip, -S, S).astype(np.int8)
    n = max(2, V // 10)
    S[V // 3:V // 3 + n] = S[V // 3]
    return S


def values_of(S):
    """the bitlevel-1 float values of a sign matrix"""
    return (np.asarray(S, np.float32) * THIRD).astype(np.float32)


def pack_signs(S):
    """uint64 [V, ceil(D / 64)] through w2b_pack_quantized: the file's layout"""
    return w2b.pack_quantized(values_of(S), 1)


def signs_of_bits(packed, D):
    packed = np.ascontiguousarray(packed, "<u8")
    bits = np.unpackbits(packed.view(np.uint8).reshape(packed.shape[0], -1), axis=1, bitorder="little")[:, :D]
    return (1 - 2 * bits.astype(np.int8)).astype(np.int8)


def write_packed_file(path, names, packed, D):
    """the .w2bp format of include/word2bits_corpus.h, bitlevel 1"""
    packed = np.ascontiguousarray(packed, "<u8")
    with open(path, "wb") as f:
        f.write(b"W2BP1 %d %d 1\n" % (packed.shape[0], D))
        for n in names:
            f.write(n + b"\n")
        f.write(packed.tobytes())
    return path


def int_scores(S, b1, b2, b3):
    """I[q, c] = sum_a (S[b2] - S[b1] + S[b3])[a] * S[c][a], int32 [nq, V].  float32 holds every partial sum exactly
    (integers below 2^24 for D < 5.5 million)."""
    S = np.asarray(S)
    T = (S[b2].astype(np.float32) - S[b1].astype(np.float32)) + S[b3].astype(np.float32)
    out = np.empty((len(b1), S.shape[0]), np.int32)
    for r0 in range(0, S.shape[0], 65536):
        out[:, r0:r0 + 65536] = np.rint(T @ S[r0:r0 + 65536].astype(np.float32).T).astype(np.int32)
    return out


def truth_from_scores(I, b1, b2, b3, k, D):
    """the answer lists: rows other than b1, b2, b3 with I > 0, I descending, equal I by ascending row, k of them,
    short lists ending in -1 / 0; score = float32(I) / float32(D)"""
    nq = I.shape[0]
    rows, scores = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float32)
    for q in range(nq):
        i = I[q].copy()
        i[[b1[q], b2[q], b3[q]]] = 0
        idx = np.flatnonzero(i > 0)
        idx = idx[np.lexsort((idx, -i[idx]))][:k]
        rows[q, :len(idx)] = idx
        scores[q, :len(idx)] = i[idx].astype(np.float32) / np.float32(D)
    return rows, scores


def truth_topk(S, b1, b2, b3, k):
    b1, b2, b3 = (np.asarray(x, np.int64) for x in (b1, b2, b3))
    return truth_from_scores(int_scores(S, b1, b2, b3), b1, b2, b3, k, np.asarray(S).shape[1])


def truth_top1(S, b1, b2, b3):
    r, d = truth_topk(S, b1, b2, b3, 1)
    return r[:, 0], d[:, 0]


class TruthModel:
    """what oracle/eval_oracle.py's transcript() asks of a model, with top1 answered by the numpy truth; names and lookup
    are those of `om`, an EvalModel of the float file of the same model"""

    def __init__(self, om):
        self.words, self.size, self.names, self.first = om.words, om.size, om.names, om.first
        self.S = np.where(om.M < 0, -1, 1).astype(np.int8)

    def lookup(self, st):
        return self.first.get(st, self.words)

    def top1(self, b1, b2, b3):
        return truth_top1(self.S, np.asarray(b1, np.int64), np.asarray(b2, np.int64), np.asarray(b3, np.int64))


def oracle_chain_scores(M, b1, b2, b3, fma):
    """The float oracle's score of EVERY row, float32 [nq, V]: vec = (M[b2] - M[b1]) + M[b3], dist += vec[a] * M[c][a]
    for a = 0..D-1 (ref src/compute-accuracy.c:155-163).  fma=False: two float32 roundings per step.  fma=True: product
    and sum are formed in the x87 extended format, whose 64-bit significand holds them exactly for these inputs, and
    rounded once to float32.  Callers check the result against the pinned oracle's top-1."""
    M = np.asarray(M, np.float32)
    vec = (M[b2] - M[b1]) + M[b3]
    dist = np.zeros((len(b1), M.shape[0]), np.float32)
    if fma:
        assert np.finfo(np.longdouble).nmant >= 63
        Ml, vl = M.astype(np.longdouble), vec.astype(np.longdouble)
        for a in range(M.shape[1]):
            dist = (dist.astype(np.longdouble) + vl[:, a:a + 1] * Ml[None, :, a]).astype(np.float32)
    else:
        for a in range(M.shape[1]):
            dist = dist + (vec[:, a:a + 1] * M[None, :, a]).astype(np.float32)
    return dist
