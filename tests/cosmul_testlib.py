"""Helpers of the 3CosMul evaluator tests: a numpy implementation of the semantics in include/word2bits_eval.h ("3CosMul"),
independent of the C twin -- the agreement counts A_i (1-bit) / the products J_i (2-bit) from codes_testlib.int_products, the
float32 sequence of the header one numpy float32 operation at a time (numpy's float32 divide is correctly rounded), the list
order from codes_testlib.truth_from_scores -- plus the models the tests run on."""
import numpy as np

import bits_testlib
import codes_testlib
from codes_testlib import int_products, truth_from_scores

EPS = np.array([0x358637BD], np.uint32).view(np.float32)[0]      # 1e-6f
assert EPS == np.float32(1e-6)


def u_planes(M, bitlevel, rows):
    """float32 [nq, V]: u of every row against rows[q].  M is the sign matrix (bitlevel 1) or the t matrix (bitlevel 2)."""
    M = np.asarray(M)
    rows = np.asarray(rows, np.int64)
    D = M.shape[1]
    J = int_products(M, rows)
    if bitlevel == 1:
        A = (D + J) // 2                                        # J = D - 2 H: the columns on which the rows agree
        assert np.array_equal(2 * A - D, J) and A.min() >= 0 and A.max() <= D
        u = A.astype(np.float32) / np.float32(D)
    else:
        w = codes_testlib.weights(M)
        cos = (J.astype(np.float32) * w[rows][:, None]) * w[None, :]
        u = (np.float32(1) + cos) * np.float32(0.5)
    assert u.dtype == np.float32
    return u


def scores(M, bitlevel, b1, b2, b3):
    """float32 [nq, V]: (u2 * u3) / (u1 + eps), every operation a float32 operation of its own"""
    u1, u2, u3 = (u_planes(M, bitlevel, b) for b in (b1, b2, b3))
    num = u2 * u3
    den = u1 + EPS
    s = num / den
    assert s.dtype == np.float32 and np.all(den > 0)
    return s


def truth_topk(M, bitlevel, b1, b2, b3, k):
    b1, b2, b3 = (np.asarray(x, np.int64) for x in (b1, b2, b3))
    return truth_from_scores(scores(M, bitlevel, b1, b2, b3), b1, b2, b3, k)


def make_model(rng, bitlevel, V, D, Q):
    """(M, packed, b): a "corr" model (its block of identical rows gives ties at the top), Q questions b = int32 [3, Q]
    among the rows below V - 2 (the first eighth with b1 == b2 == b3), and two planted rows: V - 1 is the exact negation of
    question 0's b1 (1-bit: u1 = 0, the score is u2 * u3 / eps) and V - 2 the exact negation of question 1's b2 (1-bit: u2 =
    0, score 0, no answer; 2-bit: 1 + cos lands on 0 or +-2^-23 or so)."""
    if bitlevel == 1:
        M = bits_testlib.make_signs(rng, "corr", V, D)
    else:
        M = codes_testlib.make_codes(rng, "corr", V, D)
    b = rng.integers(0, V - 2, (3, Q)).astype(np.int32)
    n = max(1, Q // 8)
    b[:, 2:2 + n] = b[0, 2:2 + n]
    M[V - 1] = -M[b[0, 0]]
    M[V - 2] = -M[b[1, 1]]
    packed = bits_testlib.pack_signs(M) if bitlevel == 1 else codes_testlib.pack_codes(M)
    return M, packed, b


def write_model(path, bitlevel, names, packed, D):
    lib = bits_testlib if bitlevel == 1 else codes_testlib
    return lib.write_packed_file(path, names, packed, D)


def host_scores(packed, D, bitlevel, b1, b2, b3, want_u=True):
    """the C twin: (u float32 [3, V] or None, scores float32 [V]) of one question against every row"""
    from word2bits_amd import _lib
    V = packed.shape[0]
    u, s = np.empty((3, V), np.float32), np.empty(V, np.float32)
    _lib.check(_lib.lib().w2b_cosmul_scores_host(packed.ctypes.data_as(_lib.u64p), V, D, bitlevel, int(b1), int(b2), int(b3),
                                                 u.ctypes.data_as(_lib.f32p) if want_u else None, s.ctypes.data_as(_lib.f32p)))
    return (u if want_u else None), s


class TruthModel(codes_testlib.TruthModel):
    """what oracle/eval_oracle.py's transcript() asks of a model, with top1 answered by the numpy 3CosMul truth; names and
    lookup are those of `om`, an EvalModel of the float file of the same model"""

    def __init__(self, om, M, bitlevel):
        super().__init__(om, M)
        self.bitlevel = bitlevel

    def top1(self, b1, b2, b3):
        r, d = truth_topk(self.T, self.bitlevel, b1, b2, b3, 1)
        return r[:, 0], d[:, 0]
