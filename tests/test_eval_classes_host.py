"""The host twin of the word-class kernels (w2b_classes_host) against an independent numpy restatement of the loop in
include/word2bits_eval.h, "word classes": every output equal, scores by bit pattern; no tolerance anywhere.  No GPU."""
import functools

import numpy as np
import pytest

from word2bits_amd import _lib
import classes_testlib as ct

V = 300
SIZES = [1, 63, 64, 65, 200]
KS = [1, 2, 5, 33, 300]


@functools.lru_cache(maxsize=None)
def model(bitlevel, D):
    M, packed = ct.make_model(np.random.default_rng(4100 + 10 * D + bitlevel), bitlevel, V, D)
    M.setflags(write=False)
    packed.setflags(write=False)
    return M, packed


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("bitlevel", [1, 2])
def test_twin_equals_the_numpy_restatement(bitlevel, D, K):
    M, packed = model(bitlevel, D)
    got = ct.host_classes(packed, D, bitlevel, K, 10)
    want = ct.numpy_classes(M, K, 10)
    assert ct.same_result(got, want)
    cls, _, T, counts, it, _ = got
    # invariants: T_out is the per-class sum of the final cls, counts are its members
    assert np.array_equal(T, np.stack([M[cls == k].sum(axis=0, dtype=np.int64) for k in range(K)]))
    assert counts.sum() == V and np.array_equal(counts, np.bincount(cls, minlength=K))
    assert 1 <= it <= 10


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_zero_iterations_return_the_start(bitlevel):
    D, K = 65, 5
    M, packed = model(bitlevel, D)
    init = np.random.default_rng(5).integers(0, K, V).astype(np.int32)
    for start, want_cls in ((None, (np.arange(V) % K).astype(np.int32)), (init, init)):
        got = ct.host_classes(packed, D, bitlevel, K, 0, start)
        assert ct.same_result(got, ct.numpy_classes(M, K, 0, start))
        assert np.array_equal(got[0], want_cls) and np.all(got[1].view(np.uint32) == 0) and got[4] == 0 and got[5] == 0
        assert np.array_equal(got[2], ct.class_sums(M, want_cls, K)[0])


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_init_and_early_stop(bitlevel):
    D, K = 200, 5
    M, packed = model(bitlevel, D)
    init = np.random.default_rng(6).integers(0, K, V).astype(np.int32)
    full = ct.host_classes(packed, D, bitlevel, K, 50, init)
    assert ct.same_result(full, ct.numpy_classes(M, K, 50, init))
    it = full[4]
    assert 1 <= it < 50 and full[5] == 0                      # it converged: the last iteration moved nothing
    assert ct.same_result(full, ct.host_classes(packed, D, bitlevel, K, it, init))
    if it > 1:                                                 # one iteration less has not stopped moving
        assert ct.host_classes(packed, D, bitlevel, K, it - 1, init)[5] > 0


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_a_dead_class_stays_empty(bitlevel):
    """init puts exactly rows 0 and 1, which are opposites, into class 2 of 3: T_2 is zero in every column"""
    D, K = 65, 3
    M, packed = model(bitlevel, D)
    assert np.array_equal(M[1], -M[0])
    init = (np.arange(V) % 2).astype(np.int32)
    init[:2] = 2
    for iters in (1, 2, 3, 10):
        got = ct.host_classes(packed, D, bitlevel, K, iters, init)
        assert ct.same_result(got, ct.numpy_classes(M, K, iters, init))
        assert not np.any(got[0] == 2) and got[3][2] == 0 and not np.any(got[2][2])


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_a_row_with_only_negative_scores_gets_the_best_live_class(bitlevel):
    """ten copies of a prototype and its negation at K = 1: the negation scores below 0 and still belongs to class 0"""
    D = 65
    M0, _ = model(bitlevel, D)
    M = np.concatenate([np.tile(M0[5], (10, 1)), -M0[5:6]]).astype(np.int8)
    got = ct.host_classes(ct.pack(M, bitlevel), D, bitlevel, 1, 3)
    assert ct.same_result(got, ct.numpy_classes(M, 1, 3))
    assert np.all(got[0] == 0) and got[1][10] < 0 and np.all(got[1][:10] > 0) and got[3][0] == 11


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_all_classes_dead_sends_every_row_to_class_0(bitlevel):
    D = 63
    M0, _ = model(bitlevel, D)
    M = np.stack([M0[3], M0[4], -M0[3], -M0[4]]).astype(np.int8)   # c % 2 pairs every row with its opposite
    got = ct.host_classes(ct.pack(M, bitlevel), D, bitlevel, 2, 5)
    assert ct.same_result(got, ct.numpy_classes(M, 2, 5))
    assert np.all(got[0] == 0) and np.all(got[1].view(np.uint32) == 0) and got[4] == 2 and got[5] == 0
    assert not np.any(got[2]) and list(got[3]) == [4, 0]


def test_refusals_leave_the_outputs_untouched():
    D, K = 65, 5
    _, packed = model(1, D)
    out = ct.outputs(V, D, K)
    EINVAL = _lib.W2B_EINVAL

    def refused(why_part, *a, **kw):
        rc, why = ct.host_classes_raw(*a, out, **kw)
        assert rc == EINVAL and why_part in why, (rc, why)
        assert ct.untouched(out)

    for bad_k in (0, -1):
        refused(b"n_classes must be at least 1", packed, D, 1, bad_k, 10, None)
        refused(b"n_classes must be at least 1", None, D, 1, bad_k, 10, None, words=V)     # no table: the n_classes is reported
    for bad_it in (-1, 1001):
        refused(b"max_iters must be 0..1000", packed, D, 1, K, bad_it, None)
    refused(b"bitlevel must be 1 or 2", packed, D, 3, K, 10, None)
    refused(b"n_classes must be at most min(words, 16384)", packed, D, 1, V + 1, 10, None)
    tiny = np.zeros((4, 1), np.uint64)                         # (every check comes before the first read of the table)
    refused(b"n_classes must be at most min(words, 16384)", tiny, 1, 1, ct.MAX_CLASSES + 1, 10, None, words=20000)
    refused(b"words must be at most 5592405", tiny, 1, 1, K, 10, None, words=ct.MAX_WORDS + 1)
    refused(b"9 * words^2 * size must stay below 2^63", tiny, 50000, 1, K, 10, None, words=5000000)
    for row, bad in ((17, K), (3, -1)):
        init = np.zeros(V, np.int32)
        init[row] = bad
        init[200] = K + 7                                      # a later offender: the first one is named
        refused(b"init: row %d: class out of range" % row, packed, D, 1, K, 10, init)
    rc, why = ct.host_classes_raw(packed, D, 1, ct.MAX_CLASSES, 0, None, ct.outputs(1, 1, 1), words=V)
    assert rc == EINVAL and b"min(words, 16384)" in why


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_planted_prototypes_are_recovered(bitlevel):
    """1000 rows x 65 columns from 5 prototypes with 20 % of the signs flipped, K = 5, 10 iterations from c % K: purity >= 0.99.
    A property of the definition, not of the code under test: the seed is one for which the numpy restatement ALONE meets
    the bound (it gives RECOVERY_PURITY below); the twin then has to give the same classes."""
    M, packed, labels = ct.planted(np.random.default_rng(SEED[bitlevel]), bitlevel, 1000, 65, 5, 0.2)
    want = ct.numpy_classes(M, 5, 10)
    p = ct.purity(want[0], labels, 5)
    print("purity of the numpy restatement at bitlevel %d: %.4f" % (bitlevel, p))
    assert p >= 0.99
    got = ct.host_classes(packed, 65, bitlevel, 5, 10)
    assert ct.same_result(got, want) and ct.purity(got[0], labels, 5) >= 0.99


SEED = {1: 3, 2: 4}
