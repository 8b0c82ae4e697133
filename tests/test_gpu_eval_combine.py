"""The signed multi-word question on the GPU (include/word2bits_eval.h, w2b_eval_combine): the bit-sliced scan of a bits
handle against the host twin, the list form of the fp32 scan against a numpy emulation of its float chain, and both
against the three-row queries they generalise.  Rows and score bits are compared exactly; no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT, write_vectors_file
from topk_testlib import same_floats, seeded_matrix
from bits_testlib import make_signs, pack_signs, write_packed_file
import codes_testlib
from combine_testlib import (bits_truth, build_vec, chain_scores, float_truth, host_scores, random_terms)

pytestmark = pytest.mark.gpu
NEAR = os.path.join(ROOT, "nearest")


def check(got, want):
    (gr, gd), (wr, wd) = got, want
    assert gr.shape == wr.shape and gd.shape == wd.shape
    assert np.array_equal(gr, wr), np.argwhere(gr != wr)[:10]
    assert same_floats(gd, wd)


def names_of(V):
    return [b"w%d" % i for i in range(V)]


def bits_handle(tmp_path, S):
    V, D = S.shape
    return w2b.Evaluator(write_packed_file(str(tmp_path / "v.w2bp"), names_of(V), pack_signs(S), D), bits=True)


def planted_terms(rng, V, nq, nt):
    """random_terms; question 0 (nt >= 2) is rows that cancel exactly: t = 0 in every column, no row has I > 0"""
    rows, signs = random_terms(rng, V, nq, nt)
    if nt >= 2:
        signs[0] = 0
        for j in range(0, nt - 1, 2):
            rows[0, j:j + 2], signs[0, j:j + 2] = rows[0, j], (1, -1)
    return rows, signs


# D = 1100 lies beyond the 1024 columns up to which the planes stay in registers (1024 itself is the last that does)
@pytest.mark.parametrize("V", [70, 300])
@pytest.mark.parametrize("D", [1, 33, 64, 65, 200, 1024, 1100])
def test_bits_equal_the_host_twin(gpu, D, V, tmp_path):
    rng = np.random.default_rng(D * 131 + V)
    S = make_signs(rng, "corr", V, D)                        # tie-heavy: a block of identical rows, near copies
    packed = pack_signs(S)
    ev = bits_handle(tmp_path, S)
    NQ = 257
    for nt in (1, 2, 4, 7):
        rows, signs = planted_terms(rng, V, NQ, nt)
        I = np.stack([host_scores(packed, D, rows[q], signs[q]) for q in range(NQ)])
        answers = np.array([np.count_nonzero(np.delete(I[q], rows[q][signs[q] != 0]) > 0) for q in range(NQ)])
        if nt >= 2:
            assert answers[0] == 0 and np.all(I[0] == 0)     # the question without an answer is really there
        if V == 70:
            assert np.any((answers > 0) & (answers < 64))    # ... and a list that ends early at k = 64
        for nq in (1, 129, 257):                             # one more than a workgroup's questions, and than two
            for k in (1, 5, 64):
                check(ev.combine(rows[:nq], signs[:nq], k), bits_truth(I[:nq], rows, signs, k, D))
    ev.close()


def test_bits_single_term_without_an_answer(gpu, tmp_path):
    """every other row is the exact opposite of row 0, or orthogonal to it (I == 0: never an answer)"""
    D, V = 70, 40
    base = make_signs(np.random.default_rng(4), "random", 1, D)[0]
    S = np.tile(-base, (V, 1)).astype(np.int8)
    S[0] = base
    S[3, :D // 2] = base[:D // 2]
    I = host_scores(pack_signs(S), D, [0], [1])
    assert I[3] == 0 and I[1:].max() == 0
    ev = bits_handle(tmp_path, S)
    for k in (1, 5):
        r, d = ev.combine([[0]], [[1]], k)
        assert np.all(r == -1) and np.all(d.view(np.uint32) == 0)
    r, d = ev.combine([[0]], [[-1]], 64)                     # the negated question: all V - 2 opposite rows, in row order
    assert list(r[0, :V - 2]) == [c for c in range(1, V) if c != 3] and np.all(r[0, V - 2:] == -1)
    ev.close()


def equivalences(ev, rng, V):
    b = rng.integers(0, V, (3, 200)).astype(np.int32)
    b[:, :20] = b[0, :20]
    three = np.stack([b[1], b[0], b[2]], 1)
    junk = np.concatenate([three[:, :1], np.full((200, 1), 2 ** 31 - 1, np.int32), three[:, 1:],
                           rng.integers(0, V, (200, 1)).astype(np.int32)], 1)
    for k in (1, 10):
        want = ev.topk(*b, k)
        check(ev.combine(three, np.tile(np.array([1, -1, 1], np.int8), (200, 1)), k), want)
        check(ev.combine(junk, np.tile(np.array([1, 0, -1, 1, 0], np.int8), (200, 1)), k), want)
        check(ev.combine(b[0][:, None], np.ones((200, 1), np.int8), k), ev.neighbors(b[0], k))
        check(ev.most_similar([[x, z] for x, z in zip(b[1], b[2])], [[y] for y in b[0]], k),
              ev.combine(np.stack([b[1], b[2], b[0]], 1), np.tile(np.array([1, 1, -1], np.int8), (200, 1)), k))


@pytest.mark.parametrize("D", [65, 200])
def test_bits_equal_the_three_row_queries(gpu, D, tmp_path):
    rng = np.random.default_rng(D)
    V = 300
    ev = bits_handle(tmp_path, make_signs(rng, "corr", V, D))
    equivalences(ev, rng, V)
    ev.close()


def f32_handle(tmp_path, rng, kind, V, D, fused):
    path = write_vectors_file(str(tmp_path / "m.bin"), names_of(V), seeded_matrix(rng, kind, V, D))
    return w2b.Evaluator(path, 0, 0, fused=fused)


@pytest.mark.parametrize("mode", ["mfma", "valu", "nofma"])
@pytest.mark.parametrize("D", [7, 200])
def test_f32_equal_the_three_row_queries(gpu, D, mode, tmp_path):
    rng = np.random.default_rng(D + 1)
    V = 300
    ev = f32_handle(tmp_path, rng, "1bit", V, D, mode != "nofma")
    if mode == "valu":
        ev.set_kernel(0)
    equivalences(ev, rng, V)
    ev.close()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kind", ["1bit", "float"])
def test_f32_general_terms_equal_the_chain(gpu, kind, fused, tmp_path):
    rng = np.random.default_rng(17)
    V, D, NQ, k = 300, 40, 24, 10
    ev = f32_handle(tmp_path, rng, kind, V, D, fused)
    M = ev.matrix()
    for nt in (2, 5, 7):
        rows, signs = random_terms(rng, V, NQ, nt)
        rows[0], signs[0] = rng.permutation(V)[:nt], 1       # all positive, all different: its own rows score highest
        rows[1, 1], signs[1, :2] = rows[1, 0], (1, 1)        # a repeated row
        dist = chain_scores(M, build_vec(M, rows, signs), fused)
        assert np.nanargmax(dist[0]) in rows[0]
        want = float_truth(dist, rows, signs, k)
        assert not np.any(np.isin(want[0][0], rows[0])) and want[0][0, 0] >= 0
        got = ev.combine(rows, signs, k)
        check(got, want)
        if fused:
            ev.set_kernel(0)
            check(ev.combine(rows, signs, k), want)
            ev.set_kernel(1)
        for q in range(NQ):
            assert not np.any(np.isin(got[0][q], rows[q][signs[q] != 0]))
    ev.close()


@pytest.mark.parametrize("bits", [True, False])
def test_scratch_bound_timing_and_argument_errors(gpu, bits, tmp_path):
    rng = np.random.default_rng(5)
    V, D, Q, k = 300, 65, 300, 10
    S = make_signs(rng, "corr", V, D)
    ev = bits_handle(tmp_path, S) if bits else f32_handle(tmp_path, rng, "1bit", V, D, True)
    rows, signs = random_terms(rng, V, Q, 5)
    ev.timing()
    want = ev.combine(rows, signs, k)
    ms, launches, macs = ev.timing()
    assert launches == 1 and ms > 0 and (macs == 1.0 * Q * V * D if bits else macs >= 1.0 * Q * V * D)
    ev.set_topk_scratch(1)                                   # one 128-question chunk per launch
    check(ev.combine(rows, signs, k), want)
    assert ev.timing()[1] == (Q + 127) // 128
    ev.set_topk_scratch(0)
    for bad in (lambda: ev.combine(rows, signs, 0), lambda: ev.combine(rows, signs, 65),
                lambda: ev.combine(np.zeros((2, 8), np.int32), np.ones((2, 8), np.int8), k),
                lambda: ev.combine(np.full((2, 2), V, np.int32), np.ones((2, 2), np.int8), k),
                lambda: ev.combine(np.zeros((2, 2), np.int32), np.full((2, 2), 2, np.int8), k),
                lambda: ev.combine(np.zeros((2, 2), np.int32), np.array([[1, 0], [0, 0]], np.int8), k)):
        with pytest.raises(w2b.W2bError) as e:
            bad()
        assert e.value.code == _lib.W2B_EINVAL
    check(ev.combine(np.array([[0, V]], np.int32), np.array([[1, 0]], np.int8), k), ev.neighbors([0], k))
    ev.close()


def listing(ev, head, rows, signs, k):
    r, d = ev.combine([rows], [signs], k)
    return head + b":\n" + b"".join(b"%d\t%s\t%s\n" % (j + 1, ev.word(r[0, j]), ("%.6f" % float(d[0, j])).encode())
                                    for j in range(k) if r[0, j] >= 0)


def test_text_form_and_command_line(gpu, tmp_path):
    rng = np.random.default_rng(12)
    V, D, k = 120, 65, 5
    path = write_packed_file(str(tmp_path / "v.w2bp"), names_of(V), pack_signs(make_signs(rng, "corr", V, D)), D)
    ev = w2b.Evaluator(path, bits=True)
    eight = b"w1 w2 w3 w4 w5 w6 w7 w8"
    queries = b"w3  w4\n+w5 -w6 +W7\n\n+w5 -nosuch -either\n" + eight + b"\n-w9"
    want = (listing(ev, b"W3 W4", [3, 4], [1, 1], k) + listing(ev, b"+W5 -W6 +W7", [5, 6, 7], [1, -1, 1], k) +
            b"+W5 -NOSUCH -EITHER: not in vocabulary: NOSUCH\n" + eight.upper() + b": expected 1 to 7 signed words\n" +
            listing(ev, b"-W9", [9], [-1], k))
    assert want.count(b"\n") > 3 * k
    assert ev.combine_text(queries, k) == want
    r = subprocess.run([NEAR, path, str(k), "0", "0", "bits", "signed"], input=queries, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    r = subprocess.run([NEAR, path, str(k), "0", "0", "bits"], input=eight + b"\n", capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == eight.upper() + b": expected 1 or 3 words\n", r.stderr
    ev.close()


def test_codes_handle_refuses(gpu, tmp_path):
    rng = np.random.default_rng(2)
    V, D = 40, 70
    T = codes_testlib.make_codes(rng, "random", V, D)
    ev = w2b.Evaluator(codes_testlib.write_packed_file(str(tmp_path / "c.w2bp"), names_of(V), codes_testlib.pack_codes(T), D),
                       codes=True)
    for call in (lambda: ev.combine([[1, 2]], [[1, -1]], 3), lambda: ev.combine_text(b"w1 w2\n", 3)):
        with pytest.raises(w2b.W2bError) as e:
            call()
        assert e.value.code == _lib.W2B_EINVAL and "not available in codes mode" in str(e.value)
    ev.close()
