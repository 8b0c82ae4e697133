"""The vector question (include/word2bits_eval.h, "vector questions"), the part that needs no GPU: the ABI, the host twin of
the kernels against an independent numpy chain (bit for bit), and every refusal with its cause."""
import ctypes as C
import os

import numpy as np
import pytest

from word2bits_amd import _lib
from w2b_testlib import ROOT
from vectors_testlib import exact_queries, host_vector, make_model, numpy_vector

DECLARATIONS = {
    "w2b_eval_vectors": """int w2b_eval_vectors(w2b_eval *e, int64_t nq, const float *x /* [nq][size], host */, int32_t normalize,
                     int32_t k, int32_t *best, float *bestd);""",
    "w2b_eval_vectors_text": """int w2b_eval_vectors_text(w2b_eval *e, const char *queries, int64_t len, int32_t normalize, int32_t k,
                          char **out, int64_t *out_len);""",
    "w2b_vector_scores_host": """int w2b_vector_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel,
                           const float *x /* [dim] */, int32_t normalize, float *S_out, float *score_out);""",
}
V = 120


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = " ".join(open(os.path.join(ROOT, "include", "word2bits_eval.h")).read().split())
    for name, text in DECLARATIONS.items():
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert " ".join(text.split()) in header, name
    i32p, i64p, f32p, vp = _lib.i32p, _lib.i64p, _lib.f32p, _lib.vp
    assert _lib.SIGNATURES["w2b_eval_vectors"] == (C.c_int, [vp, C.c_int64, f32p, C.c_int32, C.c_int32, i32p, f32p])
    assert _lib.SIGNATURES["w2b_eval_vectors_text"] == (C.c_int, [vp, C.c_char_p, C.c_int64, C.c_int32, C.c_int32,
                                                                  C.POINTER(vp), i64p])
    assert _lib.SIGNATURES["w2b_vector_scores_host"] == (C.c_int, [_lib.u64p, C.c_int64, C.c_int64, C.c_int32, f32p, C.c_int32,
                                                                   f32p, f32p])


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 3, 65, 200])
def test_host_twin_equals_the_numpy_chain(dim, bitlevel):
    rng = np.random.default_rng(100 * dim + bitlevel)
    M, packed = make_model(rng, bitlevel, V, dim)
    rounded = 0
    for x in exact_queries(rng, 6, dim):
        for normalize in (0, 1):
            rc, S, sc = host_vector(packed, dim, bitlevel, x, normalize)
            wS, wsc = numpy_vector(M, bitlevel, x, normalize)
            assert rc == 0 and same_bits(S, wS) and same_bits(sc, wsc), (dim, bitlevel, normalize)
        exact = M.astype(np.float64) @ x.astype(np.float64)
        rounded += int(np.count_nonzero(S.astype(np.float64) != exact))
    if dim >= 65:
        assert rounded > 0                                                # the chains do round: the order matters
    # either output may be NULL
    L, x = _lib.lib(), exact_queries(rng, 1, dim)[0]
    S = np.empty(V, np.float32)
    assert L.w2b_vector_scores_host(packed.ctypes.data_as(_lib.u64p), V, dim, bitlevel, x.ctypes.data_as(_lib.f32p), 1,
                                    S.ctypes.data_as(_lib.f32p), None) == 0
    assert same_bits(S, numpy_vector(M, bitlevel, x, 1)[0])
    assert L.w2b_vector_scores_host(packed.ctypes.data_as(_lib.u64p), V, dim, bitlevel, x.ctypes.data_as(_lib.f32p), 1, None,
                                    None) == 0


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_zero_vector_scores_zero(bitlevel):
    M, packed = make_model(np.random.default_rng(5), bitlevel, V, 65)
    for normalize in (0, 1):
        for zero in (np.zeros(65, np.float32), -np.zeros(65, np.float32)):
            rc, S, sc = host_vector(packed, 65, bitlevel, zero, normalize)
            assert rc == 0 and not S.view(np.uint32).any() and not sc.view(np.uint32).any()


def test_every_refusal_names_its_cause():
    L = _lib.lib()
    err = lambda: L.w2b_last_error().decode()
    M, packed = make_model(np.random.default_rng(3), 2, V, 65)
    good = exact_queries(np.random.default_rng(4), 1, 65)[0]
    for col, value in ((0, np.nan), (7, np.inf), (64, -np.inf), (33, 2.0 ** 61), (12, 2.0 ** -61), (5, -2.0 ** -61)):
        x = good.copy()
        x[col] = value
        rc, S, sc = host_vector(packed, 65, 2, x, 1)
        assert rc == _lib.W2B_EINVAL and ("column %d:" % col) in err(), (col, value, err())
        assert np.all(np.isnan(S)) and np.all(np.isnan(sc))               # nothing was written
    for value in (2.0 ** 60, -2.0 ** 60, 2.0 ** -60, 0.0, -0.0):           # the ends of the range belong to it
        x = good.copy()
        x[9] = value
        assert host_vector(packed, 65, 2, x, 0)[0] == 0
    assert host_vector(packed, 65, 3, good, 1)[0] == _lib.W2B_EINVAL and "bitlevel" in err()
    assert host_vector(packed, 65, 2, good, 2)[0] == _lib.W2B_EINVAL and "normalize" in err()

    # the device form checks what does not depend on the handle before it looks at the handle
    best = np.full((2, 3), -5, np.int32)
    x = np.zeros((2, 65), np.float32)

    def vectors(k=3, normalize=1, nq=2):
        return L.w2b_eval_vectors(None, nq, x.ctypes.data_as(_lib.f32p), normalize, k, best.ctypes.data_as(_lib.i32p), None)

    for call, what in ((lambda: vectors(k=0), "k must be 1..64"), (lambda: vectors(k=65), "k must be 1..64"),
                       (lambda: vectors(normalize=2), "normalize must be 0 or 1"), (lambda: vectors(nq=-1), "bad argument"),
                       (lambda: vectors(), "null handle")):
        assert call() == _lib.W2B_EINVAL and what in err(), (what, err())
    assert np.all(best == -5)
