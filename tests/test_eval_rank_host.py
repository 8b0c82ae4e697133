"""Rank of a given row (include/word2bits_eval.h, "rank of a given row"), the part that needs no GPU: the new ABI and the
host twin against the numpy definition of rank_testlib -- ranks and tie counts as integers, scores bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from word2bits_amd import _lib
from w2b_testlib import ROOT
from rank_testlib import CASES, V, case, host_rank, host_truth, same_bits

SYMBOLS = ["w2b_eval_rank", "w2b_eval_neighbor_rank", "w2b_rank_host", "w2b_eval_rank_text", "w2b_eval_transcript_rank"]


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_eval.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\(" % name, header), name
    assert "rank of a given row" in header


@pytest.mark.parametrize("bitlevel,D", CASES)
def test_host_twin_equals_the_numpy_definition(bitlevel, D):
    _, packed, b, g, _, (rank, tied, score) = case(bitlevel, D)
    hr, ht, hs = host_truth(packed, D, bitlevel, b, g)
    assert np.array_equal(hr, rank), np.flatnonzero(hr != rank)[:10]
    assert np.array_equal(ht, tied), np.flatnonzero(ht != tied)[:10]
    assert same_bits(hs, score)
    # rank 0 comes with tied 0 and score +0; a rank comes with a positive score
    assert np.all((tied[rank == 0] == 0)) and np.all(score[rank == 0].view(np.uint32) == 0) and np.all(score[rank > 0] > 0)
    assert rank[0] == 0                                         # the target of question 0 is one of its own rows


@pytest.mark.parametrize("bitlevel,D", CASES)
def test_cases_cover_every_kind_of_answer(bitlevel, D):
    """a condition on the recipe, not a measurement: unranked targets, targets inside and beyond the first 64 places, ties"""
    rank, tied, _ = case(bitlevel, D)[5]
    print("bitlevel %d D %d: rank 0 x%d, 1..64 x%d, > 64 x%d, tied > 0 x%d, largest rank %d" %
          (bitlevel, D, (rank == 0).sum(), ((rank >= 1) & (rank <= 64)).sum(), (rank > 64).sum(), (tied > 0).sum(), rank.max()))
    assert (rank == 0).sum() >= 3
    assert ((rank >= 1) & (rank <= 64)).sum() >= 3
    assert (rank > 64).sum() >= 3
    assert (tied > 0).sum() >= 1


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_host_twin_refusals(bitlevel):
    D = 65
    _, packed, b, g, _, _ = case(bitlevel, D)
    L = _lib.lib()
    for bad_level in (0, 3):
        assert host_rank(packed, D, bad_level, 0, 1, 2, 3) == (_lib.W2B_EINVAL, 77, 77, np.float32(7.5))
        assert b"bitlevel must be 1 or 2" in L.w2b_last_error()
    for pos in range(4):
        for bad in (-1, V):
            rows = [0, 1, 2, 3]
            rows[pos] = bad
            assert host_rank(packed, D, bitlevel, *rows) == (_lib.W2B_EINVAL, 77, 77, np.float32(7.5)), (pos, bad)
            assert b"row out of range" in L.w2b_last_error()
    # tied and score may be NULL
    r = np.full(1, 77, np.int32)
    want = host_rank(packed, D, bitlevel, *b[:, 5], g[5])
    rc = L.w2b_rank_host(packed.ctypes.data_as(_lib.u64p), V, D, bitlevel, *(int(x) for x in b[:, 5]), int(g[5]),
                         r.ctypes.data_as(_lib.i32p), None, None)
    assert rc == _lib.W2B_OK and want[0] == _lib.W2B_OK and r[0] == want[1]


def test_a_bad_question_count_is_reported_without_a_handle_or_a_device():
    L = _lib.lib()
    assert L.w2b_eval_rank(None, -1, None, None, None, None, None, None, None) == _lib.W2B_EINVAL
    assert b"w2b_eval_rank: bad argument" in L.w2b_last_error()
    assert L.w2b_eval_neighbor_rank(None, -1, None, None, None, None, None) == _lib.W2B_EINVAL
    assert L.w2b_eval_rank(None, 3, None, None, None, None, None, None, None) == _lib.W2B_EINVAL     # NULL pointers, nq > 0
    assert L.w2b_eval_rank(None, 0, None, None, None, None, None, None, None) == _lib.W2B_OK         # no question
