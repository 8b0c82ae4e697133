"""The vector question on the GPU (include/word2bits_eval.h, w2b_eval_vectors): both packed modes against the host twin's score
of every row, sorted here; against the queries it generalises (a one-row bag and a pooled bag on the packed handles, the
three-row top-k on an fp32 handle); the scratch budget, the refusals, the timing and the command line.  Rows are compared
exactly and score bits bit for bit; no tolerance anywhere.

Shape: V = 300 rows are two scan workgroups, the last 32-row tile partial, with rows past the vocabulary; Q = 40 questions are
two question tiles, the second partial (and one pair of tiles: the second tile of the pair has 8 questions).  Row lengths: 1;
2 (exactly one K step); 3 (half a padded step); 64 and 65 (a packed-word boundary); 200 (an odd number of 8-column groups).
k_vec_scan names one regime border, 512 | 513, where it starts to walk a row in chunks of 512 columns; a wavefront holds two
row tiles on both sides of it.  513 is the first size on its far side (a second chunk of one group); 1030 has two full chunks
and a third.

The scan walks the questions in pairs of 32-question tiles and a launch is (row groups) x (ranges of pairs).  Q = 40 is one pair.
test_many_pairs_per_launch tiles the 40 questions to 200 (four pairs, one workgroup range each: the offsets into the operands,
weights, bounds and slots of later pairs); test_many_pairs_per_workgroup has V = 8 000 rows and 16 480 questions (32 row groups x
129 ranges of two pairs: a workgroup carries its operand stream, its register-resident rows and, in the chunked regime, its
reloads from one pair to the next).  Both at size 200 (an odd number of groups per pair: the operand registers change roles at
every pair) and 513 (chunked), both bit levels; every copy of a question must have the list of the original."""
import os
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT, write_vectors_file
from topk_testlib import same_floats, seeded_matrix
import bits_testlib
import codes_testlib
from bag_testlib import flatten, pooled
from vectors_testlib import expected_lists, host_vector, make_model, query_weight, standard_queries

pytestmark = pytest.mark.gpu
NEAR = os.path.join(ROOT, "nearest")
V, Q = 300, 40
SIZES = [1, 2, 3, 64, 65, 200, 513, 1030]
_cache = {}


def names_of(n):
    return [b"w%d" % i for i in range(n)]


def handle(tmp_path, bitlevel, packed, D):
    lib = bits_testlib if bitlevel == 1 else codes_testlib
    path = lib.write_packed_file(str(tmp_path / ("m%d.w2bp" % bitlevel)), names_of(packed.shape[0]), packed, D)
    return w2b.Evaluator(path, bits=bitlevel == 1, codes=bitlevel == 2), path


def batch(bitlevel, D):
    """the model (column 0 the same in every row), its Q questions and the host twin's scores of every row for each question
    and either value of normalize -- computed once, never changed"""
    if (bitlevel, D) not in _cache:
        rng = np.random.default_rng(1000 * D + bitlevel)
        M, _ = make_model(rng, bitlevel, V, D)
        M[:, 0] = M[0, 0]
        packed = bits_testlib.pack_signs(M) if bitlevel == 1 else codes_testlib.pack_codes(M)
        x = standard_queries(rng, M, Q)
        full = {}
        for normalize in (0, 1):
            full[normalize] = []
            for q in range(Q):
                rc, _, sc = host_vector(packed, D, bitlevel, x[q], normalize)
                assert rc == 0
                sc.setflags(write=False)
                full[normalize].append(sc)
        for a in (M, packed, x):
            a.setflags(write=False)
        _cache[(bitlevel, D)] = (M, packed, x, full)
    return _cache[(bitlevel, D)]


def check(got, want):
    (gr, gd), (wr, wd) = got, want
    assert gr.shape == wr.shape and gd.shape == wd.shape
    assert np.array_equal(gr, wr), np.argwhere(gr != wr)[:10]
    assert same_floats(gd, wd)


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("D", SIZES)
def test_lists_equal_the_host_twin(gpu, D, bitlevel, tmp_path):
    M, packed, x, full = batch(bitlevel, D)
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    for k in (1, 10, 64):
        for normalize in (0, 1):
            want = expected_lists(full[normalize], k)
            got = ev.vectors(x, k, normalize=bool(normalize))
            check(got, want)
            for q in (Q - 4, Q - 3):                                  # the zero vector, every score < 0: the empty list
                assert np.all(got[0][q] == -1) and not got[1][q].view(np.uint32).any()
            assert got[0][Q - 1, 0] >= 0 and 7 not in got[0][Q - 2]   # a row itself has answers; its negative never the row
    if D >= 64:
        assert np.count_nonzero(expected_lists(full[1], 64)[0][:Q - 5, 63] >= 0) > Q // 2   # the lists are full ones
    ev.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("D", [200, 513])
def test_many_pairs_per_launch(gpu, D, bitlevel, tmp_path):
    M, packed, x, full = batch(bitlevel, D)
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    reps = 5                                                              # 200 questions: three full pairs and 8 questions
    for k in (1, 10, 64):
        wr, wd = expected_lists(full[1], k)
        check(ev.vectors(np.tile(x, (reps, 1)), k), (np.tile(wr, (reps, 1)), np.tile(wd, (reps, 1))))
    ev.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("D", [200, 513])
def test_many_pairs_per_workgroup(gpu, D, bitlevel, tmp_path):
    BV, BQ, reps, k = 8000, 16, 1030, 10                                  # 16 480 questions = 258 pairs
    rng = np.random.default_rng(7 * D + bitlevel)
    M = (bits_testlib.make_signs if bitlevel == 1 else codes_testlib.make_codes)(rng, "random", BV, D)
    M[:, 0] = M[0, 0]
    packed = bits_testlib.pack_signs(M) if bitlevel == 1 else codes_testlib.pack_codes(M)
    x = standard_queries(rng, M, BQ)
    scores = []
    for q in range(BQ):
        rc, _, sc = host_vector(packed, D, bitlevel, x[q], 1)
        assert rc == 0
        scores.append(sc)
    wr, wd = expected_lists(scores, k)
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    ev.timing()
    got = ev.vectors(np.tile(x, (reps, 1)), k)
    assert ev.timing()[1] == 1                                            # one launch: 32 row groups x 129 ranges of two pairs
    check(got, (np.tile(wr, (reps, 1)), np.tile(wd, (reps, 1))))
    ev.close()


@pytest.mark.parametrize("D", [3, 65, 200])
def test_bits_signs_of_a_row_equal_its_one_row_bag(gpu, D, tmp_path):
    """x = the +-1.0 signs of row r, normalize = 0: S is the exact integer I(r, c)"""
    M, packed, _, _ = batch(1, D)
    ev, _ = handle(tmp_path, 1, packed, D)
    rows = np.random.default_rng(D).integers(0, V, 50).astype(np.int32)
    x = M[rows].astype(np.float32)
    for k in (1, 10, 64):
        got, bag = ev.vectors(x, k, normalize=False), ev.bag(rows, np.arange(51), k, exclude_own=False)
        assert np.array_equal(got[0], bag[0])
        assert np.array_equal(got[0][:, 0] >= 0, np.ones(50, bool))       # the row itself scores size > 0
    ev.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_pooled_bag_as_a_vector_equals_the_bag(gpu, bitlevel, tmp_path):
    """x = (float)T of a bag of <= 12 ids, normalize = 0: every partial sum is an integer below 2^24, hence exact"""
    D = 200
    M, packed, _, _ = batch(bitlevel, D)
    rng = np.random.default_rng(17 + bitlevel)
    bags = [rng.integers(0, V, rng.integers(1, 13)).astype(np.int32) for _ in range(50)]
    x = np.stack([pooled(M, b) for b in bags]).astype(np.float32)
    ids, offsets = flatten(bags)
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    for k in (1, 10, 64):
        got, bag = ev.vectors(x, k, normalize=False), ev.bag(ids, offsets, k, exclude_own=False)
        assert np.array_equal(got[0], bag[0]), np.argwhere(got[0] != bag[0])[:10]
    ev.close()


def struck(rows, scores, out, k):
    """the first k entries of a list without the rows in `out`, padded with -1 / 0"""
    keep = ~np.isin(rows, out) & (rows >= 0)
    r, d = np.full(k, -1, np.int32), np.zeros(k, np.float32)
    n = min(k, int(keep.sum()))
    r[:n], d[:n] = rows[keep][:n], scores[keep][:n]
    return r, d


@pytest.mark.parametrize("fused,variant", [(True, 1), (True, 0), (False, 1)])
@pytest.mark.parametrize("kind", ["1bit", "float"])
def test_fp32_handle_equals_topk(gpu, kind, fused, variant, tmp_path):
    """x = float32 (M[b2] - M[b1]) + M[b3], normalize = 0: the k + 3 list with b1, b2, b3 struck out is w2b_eval_topk's"""
    D, nq = 65, 150                                                       # two 128-question tiles
    rng = np.random.default_rng(31)
    path = write_vectors_file(str(tmp_path / "m.bin"), names_of(V), seeded_matrix(rng, kind, V, D))
    ev = w2b.Evaluator(path, 0, 0, fused=fused)
    ev.set_kernel(variant)
    Mn = ev.matrix()
    b1, b2, b3 = rng.integers(0, V, (3, nq)).astype(np.int32)
    x = (Mn[b2] - Mn[b1]) + Mn[b3]
    assert x.dtype == np.float32
    for k in (1, 10):
        wr, wd = ev.topk(b1, b2, b3, k)
        gr, gd = ev.vectors(x, k + 3, normalize=False)
        for q in range(nq):
            r, d = struck(gr[q], gd[q], [b1[q], b2[q], b3[q]], k)
            assert np.array_equal(r, wr[q]) and same_floats(d, wd[q]), q
    assert np.any(ev.vectors(x, 4, normalize=False)[0] == b2[:, None])     # nothing is excluded here
    # normalize = 1 scales x by one float32 per question; the zero vector has no answers
    wx = np.array([query_weight(x[q], 1) for q in range(4)], np.float32)
    scaled = (x[:4] * wx[:, None]).astype(np.float32)
    check(ev.vectors(x[:4], 10, normalize=True), ev.vectors(scaled, 10, normalize=False))
    r, d = ev.vectors(np.zeros((1, D), np.float32), 5)
    assert np.all(r == -1) and not d.view(np.uint32).any()
    ev.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_scratch_budget_timing_and_refusals(gpu, bitlevel, tmp_path):
    D, k = 65, 10
    M, packed, x, full = batch(bitlevel, D)
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    ev.timing()
    want = ev.vectors(x, k)
    ms, launches, macs = ev.timing()
    assert launches == 1 and ms > 0 and macs == 1.0 * Q * V * D
    check(want, expected_lists(full[1], k))
    ev.set_topk_scratch(1)                                                # the smallest budget: one 32-question tile per launch
    check(ev.vectors(x, k), want)
    assert ev.timing()[1] == (Q + 31) // 32 == 2
    ev.set_topk_scratch(0)
    check(ev.vectors(x, k), want)

    best, bestd = np.full((Q, k), -5, np.int32), np.full((Q, k), -5, np.float32)
    for value in (np.nan, np.inf, 2.0 ** 61, 2.0 ** -61):
        bad = x.copy()
        bad[1, 5] = value
        rc = _lib.lib().w2b_eval_vectors(ev._h, Q, bad.ctypes.data_as(_lib.f32p), 1, k, best.ctypes.data_as(_lib.i32p),
                                         bestd.ctypes.data_as(_lib.f32p))
        assert rc == _lib.W2B_EINVAL and b"question 1, column 5:" in _lib.lib().w2b_last_error()
        assert np.all(best == -5) and np.all(bestd == -5)
    for call in (lambda: ev.vectors(x, 0), lambda: ev.vectors(x, 65), lambda: ev.vectors(x, k, normalize=2)):
        with pytest.raises(w2b.W2bError) as e:
            call()
        assert e.value.code == _lib.W2B_EINVAL
    r, d = ev.vectors(np.zeros((0, D), np.float32), k)                    # no questions
    assert r.shape == (0, k) and d.shape == (0, k)
    ev.close()


def listing(ev, head, x, k):
    r, d = ev.vectors(x, k)
    return head + b":\n" + b"".join(b"%d\t%s\t%s\n" % (j + 1, ev.word(r[0, j]), ("%.6f" % float(d[0, j])).encode())
                                    for j in range(k) if r[0, j] >= 0)


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_text_form_and_command_line(gpu, bitlevel, tmp_path):
    D, k = 3, 5
    M, packed, _, _ = batch(bitlevel, D)
    ev, path = handle(tmp_path, bitlevel, packed, D)
    queries = b"0.5 -1.25 2\n1 2\n\n1 1e30 2\n  -25e-2\t0x1p-2 7  "
    want = (listing(ev, b"vector 1", [0.5, -1.25, 2], k) + b"vector 2: expected 3 numbers\n" +
            b"vector 3: value out of range\n" + listing(ev, b"vector 4", [-0.25, 0.25, 7], k))
    assert want.count(b"\n") > k
    assert ev.vectors_text(queries, k) == want
    assert ev.vectors_text(b"1 two 3\n", k) == b"vector 1: expected 3 numbers\n"
    r = subprocess.run([NEAR, path, str(k), "0", "0", "bits" if bitlevel == 1 else "codes", "vector"], input=queries,
                       capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    ev.close()
