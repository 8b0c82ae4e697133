"""3CosMul scoring (include/word2bits_eval.h, "3CosMul"), the part that needs no GPU: the new ABI and the host twin of the
kernels against the numpy definition of cosmul_testlib, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from word2bits_amd import _lib
from w2b_testlib import ROOT
from cosmul_testlib import EPS, host_scores, make_model, scores, u_planes

SYMBOLS = ["w2b_eval_cosmul", "w2b_eval_cosmul_text", "w2b_eval_transcript_cosmul", "w2b_cosmul_scores_host"]
V, Q = 300, 40


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_eval.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\(" % name, header), name
    assert EPS.view(np.uint32) == 0x358637BD and "0x358637BD" in header


def bits_of(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("D", [1, 3, 64, 65, 200])
@pytest.mark.parametrize("bitlevel", [1, 2])
def test_host_twin_equals_the_numpy_definition(bitlevel, D):
    rng = np.random.default_rng(4000 + 10 * D + bitlevel)
    M, packed, b = make_model(rng, bitlevel, V, D, Q)
    S = scores(M, bitlevel, *b)
    U = [u_planes(M, bitlevel, b[i]) for i in range(3)]
    for q in range(Q):
        u, s = host_scores(packed, D, bitlevel, *b[:, q])
        for i in range(3):
            assert np.array_equal(bits_of(u[i]), bits_of(U[i][q])), (q, i)
        assert np.array_equal(bits_of(s), bits_of(S[q])), q
        _, s_only = host_scores(packed, D, bitlevel, *b[:, q], want_u=False)
        assert np.array_equal(bits_of(s_only), bits_of(s))
        # the two positives commute: one float32 product
        _, swapped = host_scores(packed, D, bitlevel, b[0, q], b[2, q], b[1, q])
        assert np.array_equal(bits_of(swapped), bits_of(s)), q
    # the planted rows: V - 1 negates question 0's b1, V - 2 negates question 1's b2
    if bitlevel == 1:
        u, s = host_scores(packed, D, 1, *b[:, 0])
        assert u[0, V - 1] == 0 and bits_of(s[V - 1]) == bits_of((u[1, V - 1] * u[2, V - 1]) / EPS)
        u, s = host_scores(packed, D, 1, *b[:, 1])
        assert u[1, V - 2] == 0 and bits_of(s[V - 2]) == 0
    else:
        u, _ = host_scores(packed, D, 2, *b[:, 1])
        assert abs(float(u[1, V - 2])) <= 2.0 ** -23            # (1 + cos) / 2 with cos within an ulp or two of -1
    assert np.all(np.isfinite(S)) and not np.any((S != 0) & (np.abs(S) < np.finfo(np.float32).tiny))


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_host_twin_refusals(bitlevel):
    rng = np.random.default_rng(7)
    D = 65
    M, packed, b = make_model(rng, bitlevel, V, D, Q)
    L = _lib.lib()
    p = packed.ctypes.data_as(_lib.u64p)
    s = np.full(V, 7.0, np.float32)
    sp = s.ctypes.data_as(_lib.f32p)
    assert L.w2b_cosmul_scores_host(p, V, D, 3, 0, 1, 2, None, sp) == _lib.W2B_EINVAL and b"bitlevel" in L.w2b_last_error()
    assert L.w2b_cosmul_scores_host(p, V, D, 0, 0, 1, 2, None, sp) == _lib.W2B_EINVAL
    for bad in ((V, 0, 0), (0, V, 0), (0, 0, V), (0, -1, 0), (V + 5, 1, 2)):
        assert L.w2b_cosmul_scores_host(p, V, D, bitlevel, *bad, None, sp) == _lib.W2B_EINVAL
        assert b"row out of range" in L.w2b_last_error()
    assert np.all(s == 7.0)                                    # refused: nothing written
    assert L.w2b_cosmul_scores_host(p, V, D, bitlevel, 0, 1, 2, None, None) == _lib.W2B_OK
