"""The bag question on the GPU (include/word2bits_eval.h, w2b_eval_bag): both packed modes against the host twin's J / score
of every row, sorted here; against the queries it generalises (the all-plus combine of a bits handle, the neighbours of a
codes handle); the scratch budget, the refusals, the command line and the timing.  Rows are compared exactly and score
bits bit for bit; no tolerance anywhere.

Shape: V = 300 rows are two scan workgroups at two row tiles per wavefront, the last tile partial, with rows past the
vocabulary; Q = 40 questions are two question tiles, the second partial.  Row lengths: 1; 65 (a last K step of one
column); 200; 417 (the first length with one row tile per wavefront); 1250 (the first chunked regime past 1216).  The
register report left the regime borders of k_codes_scan where they were."""
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
from bag_testlib import MAX_BAG, answer_list, flatten, host_bag, make_model, standard_bags

pytestmark = pytest.mark.gpu
NEAR = os.path.join(ROOT, "nearest")
V, Q = 300, 40
SIZES = [1, 65, 200, 417, 1250]
_cache = {}


def names_of(n):
    return [b"w%d" % i for i in range(n)]


def handle(tmp_path, bitlevel, packed, D):
    lib = bits_testlib if bitlevel == 1 else codes_testlib
    path = lib.write_packed_file(str(tmp_path / ("m%d.w2bp" % bitlevel)), names_of(packed.shape[0]), packed, D)
    return w2b.Evaluator(path, bits=bitlevel == 1, codes=bitlevel == 2), path


def batch(bitlevel, D):
    """the model, its Q bags and the host twin's (J, score) of every row for each bag -- computed once, never changed"""
    if (bitlevel, D) not in _cache:
        rng = np.random.default_rng(1000 * D + bitlevel)
        M, packed = make_model(rng, bitlevel, V, D)
        bags = standard_bags(rng, V)
        bags += [np.array([5, -1, 9, -1, -1, 200], np.int32), np.array([7, 7, 7, 30, 7], np.int32),
                 rng.integers(0, V, MAX_BAG).astype(np.int32)]
        bags += [rng.integers(0, V, rng.integers(1, 13)).astype(np.int32) for _ in range(Q - len(bags))]
        assert len(bags) == Q
        full = []
        for b in bags:
            rc, J, sc = host_bag(packed, D, bitlevel, b)
            assert rc == 0
            full.append((J, sc))
        for a in (packed, *bags, *(x for f in full for x in f)):
            a.setflags(write=False)
        _cache[(bitlevel, D)] = (M, packed, bags, full)
    return _cache[(bitlevel, D)]


def expected(bitlevel, bags, full, k, exclude):
    rows, out = np.empty((len(bags), k), np.int32), np.empty((len(bags), k), np.float32)
    for q, (b, (J, sc)) in enumerate(zip(bags, full)):
        rows[q], out[q] = answer_list(J if bitlevel == 1 else sc, sc, b[b >= 0] if exclude else [], k)
    return rows, out


def check(got, want):
    (gr, gd), (wr, wd) = got, want
    assert gr.shape == wr.shape and gd.shape == wd.shape
    assert np.array_equal(gr, wr), np.argwhere(gr != wr)[:10]
    assert same_floats(gd, wd)


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("D", SIZES)
def test_lists_equal_the_host_twin(gpu, D, bitlevel, tmp_path):
    M, packed, bags, full = batch(bitlevel, D)
    ids, offsets = flatten(bags)
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    assert ev.is_bits == (bitlevel == 1) and ev.is_codes == (bitlevel == 2)
    for k in (1, 10, 64):
        for exclude in (False, True):
            want = expected(bitlevel, bags, full, k, exclude)
            got = ev.bag(ids, offsets, k, exclude_own=exclude)
            check(got, want)
            for q in (0, 1, 6):                                       # empty, padding only, T == 0: the empty list
                assert np.all(got[0][q] == -1) and not got[1][q].view(np.uint32).any()
    if D >= 65:
        assert np.any(expected(bitlevel, bags, full, 64, False)[0][:, 0] >= 0)
    if bitlevel == 1 and D == 1:
        assert expected(1, bags, full, 64, False)[0][2, 63] >= 0          # massive ties: the row order decides
    ev.close()


@pytest.mark.parametrize("D", [65, 200])
def test_bits_short_bags_equal_the_all_plus_combine(gpu, D, tmp_path):
    M, packed, _, _ = batch(1, D)
    rng = np.random.default_rng(D)
    ev, _ = handle(tmp_path, 1, packed, D)
    lens = rng.integers(1, 8, 60)
    rows = rng.integers(0, V, (60, 7)).astype(np.int32)
    rows[:10, 1] = rows[:10, 0]                                           # repeated rows
    lens[:10] = np.maximum(lens[:10], 2)
    signs = (np.arange(7)[None, :] < lens[:, None]).astype(np.int8)
    ids, offsets = flatten([rows[q, :lens[q]] for q in range(60)])
    for k in (1, 10):
        check(ev.bag(ids, offsets, k, exclude_own=True), ev.combine(rows, signs, k))
    ev.close()


@pytest.mark.parametrize("D", [65, 417])
def test_codes_one_row_bags_equal_the_neighbours(gpu, D, tmp_path):
    M, packed, _, _ = batch(2, D)
    ev, _ = handle(tmp_path, 2, packed, D)
    rows = np.random.default_rng(D).integers(0, V, 50).astype(np.int32)
    for k in (1, 10):
        check(ev.bag(rows, np.arange(51), k, exclude_own=True), ev.neighbors(rows, k))
    ev.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_scratch_budget_timing_and_refusals(gpu, bitlevel, tmp_path):
    D, k = 65, 10
    M, packed, bags, full = batch(bitlevel, D)
    ids, offsets = flatten(bags)
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    ev.timing()
    want = ev.bag(ids, offsets, k)
    ms, launches, macs = ev.timing()
    assert launches == 1 and ms > 0 and macs == 2.0 * Q * V * D
    ev.set_topk_scratch(1)                                                # the smallest budget: one 32-question tile per launch
    check(ev.bag(ids, offsets, k), want)
    assert ev.timing()[1] == (Q + 31) // 32 == 2
    ev.set_topk_scratch(0)
    check(ev.bag(ids, offsets, k), want)

    best, bestd = np.full((2, k), -5, np.int32), np.full((2, k), -5, np.float32)
    bad = np.array([3, V, 4], np.int32)
    two = np.array([0, 2, 3], np.int64)
    rc = _lib.lib().w2b_eval_bag(ev._h, 3, bad.ctypes.data_as(_lib.i32p), 2, two.ctypes.data_as(_lib.i64p), 1, k,
                                 best.ctypes.data_as(_lib.i32p), bestd.ctypes.data_as(_lib.f32p))
    assert rc == _lib.W2B_EINVAL and b"out of range" in _lib.lib().w2b_last_error()
    assert np.all(best == -5) and np.all(bestd == -5)
    for call in (lambda: ev.bag([0], [0, 1], 0), lambda: ev.bag([0], [0, 1], 65), lambda: ev.bag([0], [0, 1], k, exclude_own=2),
                 lambda: ev.bag(np.zeros(MAX_BAG + 1, np.int32), [0, MAX_BAG + 1], k), lambda: ev.bag([0, 1], [0, 1], k)):
        with pytest.raises(w2b.W2bError) as e:
            call()
        assert e.value.code == _lib.W2B_EINVAL
    r, d = ev.bag([], [0], k)                                             # no questions
    assert r.shape == (0, k) and d.shape == (0, k)
    if bitlevel == 2:                                                     # unchanged: the signed combine has no codes form
        with pytest.raises(w2b.W2bError) as e:
            ev.combine([[1, 2]], [[1, 1]], 3)
        assert e.value.code == _lib.W2B_EINVAL and "not available in codes mode" in str(e.value)
    ev.close()


def test_fp32_handle_refuses(gpu, tmp_path):
    rng = np.random.default_rng(8)
    path = write_vectors_file(str(tmp_path / "m.bin"), names_of(40), seeded_matrix(rng, "1bit", 40, 20))
    ev = w2b.Evaluator(path, 0, 0)
    for call in (lambda: ev.bag([1, 2], [0, 2], 3), lambda: ev.bag_text(b"w1 w2\n", 3)):
        with pytest.raises(w2b.W2bError) as e:
            call()
        assert e.value.code == _lib.W2B_EINVAL and "bits or a codes handle" in str(e.value)
    ev.close()


def listing(ev, head, rows, k):
    r, d = ev.bag(rows, [0, len(rows)], k, exclude_own=True)
    return head + b":\n" + b"".join(b"%d\t%s\t%s\n" % (j + 1, ev.word(r[0, j]), ("%.6f" % float(d[0, j])).encode())
                                    for j in range(k) if r[0, j] >= 0)


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_text_form_and_command_line(gpu, bitlevel, tmp_path):
    D, k = 65, 5
    M, packed, _, _ = batch(bitlevel, D)
    ev, path = handle(tmp_path, bitlevel, packed, D)
    ten = list(range(40, 50))
    queries = b"w3\n" + b" ".join(b"w%d" % i for i in ten) + b"\nw5 nosuch w6 either\n\nW8  w9"
    want = (listing(ev, b"W3", [3], k) + listing(ev, b" ".join(b"W%d" % i for i in ten), ten, k) +
            b"W5 NOSUCH W6 EITHER: not in vocabulary: NOSUCH\n" + listing(ev, b"W8 W9", [8, 9], k))
    assert want.count(b"\n") > 2 * k
    assert ev.bag_text(queries, k) == want
    long_line = b" ".join([b"w1"] * (MAX_BAG + 1))
    assert ev.bag_text(long_line + b"\n", k) == long_line.upper() + b": expected 1 to 4096 words\n"
    r = subprocess.run([NEAR, path, str(k), "0", "0", "bits" if bitlevel == 1 else "codes", "bag"], input=queries,
                       capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    ev.close()
