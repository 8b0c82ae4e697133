"""Helpers of the document-question tests (include/word2bits_eval.h, "documents"): the host twin, an independent numpy
restatement of the definition on the integer matrix M that it is checked against, the answer lists that the scores of every
document imply, and corpus generators."""
import numpy as np

from word2bits_amd import _lib
import bag_testlib
import codes_testlib

MAX_DOC = 1024
make_model = bag_testlib.make_model
flatten = bag_testlib.flatten


def host_docs(packed, D, bitlevel, ids, offsets, qids, symmetric, want_dir=True, want_score=True):
    """w2b_docs_scores_host for one query: (rc, dir int64 [2, n_docs], score float32 [n_docs])"""
    packed, ids = np.ascontiguousarray(packed, np.uint64), np.ascontiguousarray(ids, np.int32)
    offsets, qids = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(qids, np.int32)
    n = max(len(offsets) - 1, 0)
    R, sc = np.full((2, n), -77, np.int64), np.full(n, np.nan, np.float32)
    rc = _lib.lib().w2b_docs_scores_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0], D, bitlevel, len(ids),
                                         ids.ctypes.data_as(_lib.i32p), n, offsets.ctypes.data_as(_lib.i64p), len(qids),
                                         qids.ctypes.data_as(_lib.i32p), int(symmetric),
                                         R.ctypes.data_as(_lib.i64p) if want_dir else None,
                                         sc.ctypes.data_as(_lib.f32p) if want_score else None)
    return rc, R, sc


def pair_values(M, bitlevel, rows):
    """int64 [len(rows), V]: I (bitlevel 1) or F = ldexp(cos, 50) (bitlevel 2) of the given rows against every row, from an
    integer matmul, the weights of codes_testlib and two float32 multiplies; asserts that every F is integral"""
    M = np.asarray(M, np.int64)
    rows = np.asarray(rows, np.int64)
    J = M[rows] @ M.T
    if bitlevel == 1:
        return J
    w = codes_testlib.weights(M)
    p = J.astype(np.float32) * w[rows][:, None]
    cos = p * w[None, :]
    assert p.dtype == np.float32 and cos.dtype == np.float32
    assert not np.isnan(cos).any() and not (np.signbit(cos) & (cos == 0)).any()      # never NaN, never -0
    F = np.ldexp(cos.astype(np.float64), 50)
    assert np.array_equal(F, np.rint(F)) and np.abs(F).max(initial=0) < 2.0 ** 51
    return F.astype(np.int64)


def numpy_docs(M, bitlevel, docs, q, symmetric):
    """the definition: (dir int64 [2, n_docs], score float32 [n_docs]) of the query q (an id array) against the id arrays docs"""
    D = np.asarray(M).shape[1]
    q = np.asarray(q, np.int64)
    q = q[q >= 0]
    P = pair_values(M, bitlevel, q) if len(q) else np.zeros((0, len(M)), np.int64)
    R, sc = np.zeros((2, len(docs)), np.int64), np.zeros(len(docs), np.float32)
    for d, doc in enumerate(docs):
        doc = np.asarray(doc, np.int64)
        doc = doc[doc >= 0]
        if not len(q) or not len(doc):
            continue
        S = P[:, doc]
        R[0, d], R[1, d] = S.max(axis=1).sum(), S.max(axis=0).sum()
        s = [one_score(bitlevel, R[0, d], len(q), D), one_score(bitlevel, R[1, d], len(doc), D)]
        sc[d] = min(s) if symmetric else s[0]
    return R, sc


def one_score(bitlevel, total, m, D):
    if bitlevel == 1:
        assert abs(int(total)) < 2 ** 31 and m * D < 2 ** 31
        return np.float32(np.int32(total)) / np.float32(np.int32(m * D))
    return np.float32(np.int64(total)) / (np.float32(m) * np.float32(2.0 ** 50))


def answer_list(score, k):
    """one query's list from the scores of EVERY document: score > 0, descending, equal scores by ascending index"""
    return bag_testlib.answer_list(score, score, [], k)


def make_docs(rng, V, n_docs, lengths, pad=0.1):
    """n_docs id arrays with lengths drawn from `lengths` (every one of them at least once when n_docs allows), ids
    sprinkled with padding, some ids repeated, the first document with a length > 0 all padding"""
    lens = np.concatenate([np.array(lengths), rng.choice(lengths, max(n_docs - len(lengths), 0))])[:n_docs]
    lens = rng.permutation(lens)
    docs = []
    for n in lens:
        d = rng.integers(0, V, n).astype(np.int32)
        if n >= 2:
            d[rng.integers(0, n)] = d[0]                                  # a repeated id
        d[rng.random(n) < pad] = -1
        docs.append(d)
    for d in docs:
        if len(d):
            d[:] = -1
            break
    return docs
