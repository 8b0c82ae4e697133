"""The signed multi-word question (include/word2bits_eval.h, w2b_eval_combine), the part that needs no GPU: the new ABI
and the host twin of the bit-sliced scan against the numpy definition."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from word2bits_amd import _lib
from w2b_testlib import ROOT
from bits_testlib import make_signs, pack_signs
from combine_testlib import MAX_TERMS, host_scores, numpy_scores, random_terms


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_eval.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert re.search(r"#define W2B_EVAL_MAX_TERMS 7\b", header)
    want = {
        "w2b_eval_combine": ("int w2b_eval_combine(w2b_eval *e, int64_t nq, int32_t nt, const int32_t *rows, const int8_t "
                             "*signs, int32_t k, int32_t *best, float *bestd);",
                             [_lib.vp, C.c_int64, C.c_int32, _lib.i32p, _lib.i8p, C.c_int32, _lib.i32p, _lib.f32p]),
        "w2b_eval_combine_text": ("int w2b_eval_combine_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char "
                                  "**out, int64_t *out_len);",
                                  [_lib.vp, C.c_char_p, C.c_int64, C.c_int32, C.POINTER(_lib.vp), _lib.i64p]),
        "w2b_bits_combine_scores_host": ("int w2b_bits_combine_scores_host(const uint64_t *packed, int64_t words, int64_t dim, "
                                         "int32_t nt, const int32_t *rows, const int8_t *signs, int32_t *I_out);",
                                         [_lib.u64p, C.c_int64, C.c_int64, C.c_int32, _lib.i32p, _lib.i8p, _lib.i32p]),
    }
    for name, (decl, args) in want.items():
        assert hasattr(lib, name), name
        assert decl in flat, name
        assert _lib.SIGNATURES[name] == (C.c_int, args), name
    assert "not available in codes mode" in header


@pytest.mark.parametrize("D", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("nt", range(1, MAX_TERMS + 1))
def test_host_twin_equals_the_numpy_definition(D, nt):
    rng = np.random.default_rng(500 * D + nt)
    V, Q = 120, 16
    S = make_signs(rng, "corr", V, D)
    packed = pack_signs(S)
    rows, signs = random_terms(rng, V, Q, nt)
    rows[0], signs[0] = rows[0, 0], 1                        # one row nt times: its coefficients add
    signs[1] = -1                                            # all negative
    if nt % 2 == 0:                                          # even nt, every slot used: t = 0 wherever the rows cancel
        signs[2] = np.tile(np.array([1, -1], np.int8), nt // 2)
        t = (signs[2].astype(np.int64)[:, None] * S[rows[2]]).sum(0)
        assert D < 60 or np.any(t == 0)
    if nt >= 2:
        rows[3, :2], signs[3, :2] = rows[3, 0], (1, -1)      # a row against itself
    for q in range(Q):
        assert np.array_equal(host_scores(packed, D, rows[q], signs[q]), numpy_scores(S, rows[q], signs[q])), q
    assert np.array_equal(host_scores(packed, D, rows[0], signs[0]), nt * (S.astype(np.int64) @ S[rows[0, 0]]))


@pytest.mark.parametrize("D", [1, 65, 200])
def test_three_slots_equal_the_three_row_twin(D):
    rng = np.random.default_rng(D)
    V = 90
    packed = pack_signs(make_signs(rng, "corr", V, D))
    L = _lib.lib()
    for b1, b2, b3 in rng.integers(0, V, (12, 3)):
        want = np.empty(V, np.int32)
        _lib.check(L.w2b_bits_scores_host(packed.ctypes.data_as(_lib.u64p), V, D, int(b1), int(b2), int(b3),
                                          want.ctypes.data_as(_lib.i32p)))
        assert np.array_equal(host_scores(packed, D, [b2, b1, b3], [1, -1, 1]), want)
        assert np.array_equal(host_scores(packed, D, [b2, 77777, b1, b3, -5], [1, 0, -1, 1, 0]), want)   # unused slots: any row


def test_bad_arguments_are_refused_with_their_cause():
    rng = np.random.default_rng(3)
    V, D = 20, 70
    packed = pack_signs(make_signs(rng, "random", V, D))
    L = _lib.lib()
    out = np.empty(V, np.int32)

    def call(nt, rows, signs):
        rows, signs = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(signs, np.int8)
        rc = L.w2b_bits_combine_scores_host(packed.ctypes.data_as(_lib.u64p), V, D, nt, rows.ctypes.data_as(_lib.i32p),
                                            signs.ctypes.data_as(_lib.i8p), out.ctypes.data_as(_lib.i32p))
        return rc, L.w2b_last_error().decode()

    assert call(2, [1, 2], [1, -1])[0] == _lib.W2B_OK
    for nt in (0, 8, -1):
        rc, why = call(nt, [1] * 8, [1] * 8)
        assert rc == _lib.W2B_EINVAL and "number of terms" in why, (nt, why)
    for bad in (2, -2, 100):
        rc, why = call(2, [1, 2], [1, bad])
        assert rc == _lib.W2B_EINVAL and "sign" in why, (bad, why)
    for bad in (-1, V, 2 ** 31 - 1):
        rc, why = call(3, [1, bad, 2], [1, -1, 1])
        assert rc == _lib.W2B_EINVAL and "row out of range" in why, (bad, why)
        assert call(3, [1, bad, 2], [1, 0, 1])[0] == _lib.W2B_OK          # an unused slot's row is ignored
    rc, why = call(3, [1, 2, 3], [0, 0, 0])
    assert rc == _lib.W2B_EINVAL and "at least one" in why, why
