"""The bag question (include/word2bits_eval.h, "bag questions"), the part that needs no GPU: the ABI, the host twin of the
kernels against a numpy definition (the pooled vector from unpacked rows, int64 products, the float32 steps one at a
time; bit for bit), its agreement with the host twins it generalises, and every refusal with its cause."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from word2bits_amd import _lib
from w2b_testlib import ROOT
import bits_testlib
import codes_testlib
from combine_testlib import host_scores as combine_host_scores
from bag_testlib import MAX_BAG, flatten, host_bag, make_model, numpy_bag, pooled, standard_bags

DECLARATIONS = {
    "w2b_eval_bag": """int w2b_eval_bag(w2b_eval *e, int64_t n_ids, const int32_t *ids, int64_t nq, const int64_t *offsets,
                 int32_t exclude_own, int32_t k, int32_t *best, float *bestd);""",
    "w2b_eval_bag_text": """int w2b_eval_bag_text(w2b_eval *e, const char *queries, int64_t len, int32_t exclude_own, int32_t k,
                      char **out, int64_t *out_len);""",
    "w2b_bag_scores_host": """int w2b_bag_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel,
                        int64_t n, const int32_t *ids, int32_t *J_out, float *score_out);""",
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
    assert re.search(r"#define W2B_EVAL_MAX_BAG 4096\b", header) and MAX_BAG == 4096
    i32p, i64p, f32p, vp = _lib.i32p, _lib.i64p, _lib.f32p, _lib.vp
    assert _lib.SIGNATURES["w2b_eval_bag"] == (C.c_int, [vp, C.c_int64, i32p, C.c_int64, i64p, C.c_int32, C.c_int32, i32p, f32p])
    assert _lib.SIGNATURES["w2b_bag_scores_host"] == (C.c_int, [_lib.u64p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, i32p, i32p,
                                                               f32p])


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 200])
def test_host_twin_equals_the_numpy_definition(dim, bitlevel):
    rng = np.random.default_rng(100 * dim + bitlevel)
    M, packed = make_model(rng, bitlevel, V, dim)
    bags = standard_bags(rng, V)
    assert [len(b) for b in bags] == [0, 5, 1, 7, 300, MAX_BAG, 2]
    T300, Tmax, Tzero = pooled(M, bags[4]), pooled(M, bags[5]), pooled(M, bags[6])
    assert np.abs(T300).max() > 127                                       # the high digit is used
    assert set(np.abs(Tmax).tolist()) <= ({4096} if bitlevel == 1 else {4096, 12288}) and not Tzero.any()
    for ids in bags:
        rc, J, sc = host_bag(packed, dim, bitlevel, ids)
        wJ, wsc = numpy_bag(M, bitlevel, ids)
        assert rc == 0 and np.array_equal(J, wJ) and same_bits(sc, wsc), len(ids)
        if not pooled(M, ids).any():
            assert not J.any() and not sc.view(np.uint32).any()           # every score is +0
    # either output may be NULL
    L, ids = _lib.lib(), bags[3]
    J = np.empty(V, np.int32)
    assert L.w2b_bag_scores_host(packed.ctypes.data_as(_lib.u64p), V, dim, bitlevel, 7, ids.ctypes.data_as(_lib.i32p),
                                 J.ctypes.data_as(_lib.i32p), None) == 0
    assert np.array_equal(J, numpy_bag(M, bitlevel, ids)[0])
    assert L.w2b_bag_scores_host(packed.ctypes.data_as(_lib.u64p), V, dim, bitlevel, 7, ids.ctypes.data_as(_lib.i32p), None,
                                 None) == 0


@pytest.mark.parametrize("dim", [1, 65, 200])
def test_pooled_vector_is_that_of_the_embedding_layer(dim):
    """T == 4 * the SUM of w2b_embed_bag_host at bitlevel 2, exactly"""
    rng = np.random.default_rng(dim)
    M, packed = make_model(rng, 2, V, dim)
    ids, offsets = flatten(standard_bags(rng, V))
    out = np.full((len(offsets) - 1, dim), np.nan, np.float32)
    assert _lib.lib().w2b_embed_bag_host(packed.ctypes.data_as(_lib.u64p), V, dim, 2, len(ids), ids.ctypes.data_as(_lib.i32p),
                                         len(offsets) - 1, offsets.ctypes.data_as(_lib.i64p), 0, out.ctypes.data_as(_lib.f32p)) == 0
    for b in range(len(offsets) - 1):
        T = pooled(M, ids[offsets[b]:offsets[b + 1]])
        assert np.array_equal(out[b].astype(np.float64) * 4, T.astype(np.float64))


@pytest.mark.parametrize("dim", [1, 65, 200])
def test_bits_bag_is_the_all_plus_combine(dim):
    rng = np.random.default_rng(dim + 7)
    M, packed = make_model(rng, 1, V, dim)
    for m in (1, 2, 7):
        rows = rng.integers(0, V, m).astype(np.int32)
        rows[-1] = rows[0]                                                # a repeated row adds
        rc, J, _ = host_bag(packed, dim, 1, rows)
        assert rc == 0 and np.array_equal(J, combine_host_scores(packed, dim, rows, np.ones(m, np.int8)))


@pytest.mark.parametrize("dim", [1, 65, 200])
def test_codes_bag_of_one_row_is_the_neighbour_score(dim):
    rng = np.random.default_rng(dim + 9)
    M, packed = make_model(rng, 2, V, dim)
    for r in (0, 17, V - 1):
        rc, J, sc = host_bag(packed, dim, 2, [r])
        J3, want = np.empty((3, V), np.int32), np.empty(V, np.float32)
        _lib.check(_lib.lib().w2b_codes_scores_host(packed.ctypes.data_as(_lib.u64p), V, dim, r, r, r,
                                                    J3.ctypes.data_as(_lib.i32p), want.ctypes.data_as(_lib.f32p)))
        assert rc == 0 and np.array_equal(J, J3[0]) and same_bits(sc, want)


def test_every_refusal_names_its_cause():
    L = _lib.lib()
    err = lambda: L.w2b_last_error().decode()
    M, packed = make_model(np.random.default_rng(3), 2, V, 65)
    one = packed[:, :1].copy()
    for ids, bitlevel, what in (([0, V], 2, "out of range"), (np.zeros(MAX_BAG + 1, np.int32), 2, "at most 4096"),
                                ([0, 1], 3, "bitlevel"), ([0, V], 1, "out of range")):
        rc, J, sc = host_bag(packed if bitlevel != 1 else one, 65 if bitlevel != 1 else 64, bitlevel, ids)
        assert rc == _lib.W2B_EINVAL and what in err(), (what, err())
        assert np.all(J == -77) and np.all(np.isnan(sc))                  # nothing was written
    rc, _, _ = host_bag(np.zeros((1, 2 * 911), np.uint64), 58255, 2, [0])
    assert rc == _lib.W2B_EINVAL and "58254" in err()
    assert host_bag(np.zeros((1, 911), np.uint64), 58254, 1, [0])[0] == 0

    # the device form checks what does not depend on the handle before it looks at the handle
    best = np.full((2, 3), -5, np.int32)
    ids = np.array([0, 1, 2], np.int32)

    def bag(offsets, k=3, exclude=1, n_ids=3):
        offsets = np.asarray(offsets, np.int64)
        return L.w2b_eval_bag(None, n_ids, ids.ctypes.data_as(_lib.i32p), len(offsets) - 1, offsets.ctypes.data_as(_lib.i64p),
                              exclude, k, best.ctypes.data_as(_lib.i32p), None)

    for call, what in ((lambda: bag([0, 2, 3], k=0), "k must be 1..64"), (lambda: bag([0, 2, 3], k=65), "k must be 1..64"),
                       (lambda: bag([0, 2, 3], exclude=2), "exclude_own"), (lambda: bag([1, 2, 3]), "offsets"),
                       (lambda: bag([0, 2, 2]), "offsets"), (lambda: bag([0, 3, 2, 3]), "offsets"),
                       (lambda: bag([0, 2, 3]), "null handle")):
        assert call() == _lib.W2B_EINVAL and what in err(), (what, err())
    long_ids = np.zeros(MAX_BAG + 1, np.int32)
    offsets = np.array([0, MAX_BAG + 1], np.int64)
    assert L.w2b_eval_bag(None, MAX_BAG + 1, long_ids.ctypes.data_as(_lib.i32p), 1, offsets.ctypes.data_as(_lib.i64p), 1, 3,
                          best.ctypes.data_as(_lib.i32p), None) == _lib.W2B_EINVAL and "at most 4096" in err()
    assert np.all(best == -5)
