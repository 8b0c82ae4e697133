"""Codes-mode evaluator on the GPU (include/word2bits_eval.h, "codes mode"): rows and score bits exactly equal to the numpy
implementation of the stated semantics (codes_testlib), which tests/test_eval_codes_host.py ties to the pinned float
oracle; no tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT, eval_oracle, write_vectors_file
from topk_testlib import same_floats
from bits_testlib import make_signs, pack_signs
from bits_testlib import write_packed_file as write_packed_file_1bit
from codes_testlib import (TruthModel, codes_of_packed, float_bound, lead_over_runner_up, make_codes, pack_codes, scores,
                           truth_from_scores, truth_topk, values_of, write_packed_file)

pytestmark = pytest.mark.gpu
ACC, NEAR, W2B = (os.path.join(ROOT, n) for n in ("compute_accuracy", "nearest", "word2bits"))


def check(got, want):
    (gr, gd), (wr, wd) = got, want
    assert gr.shape == wr.shape and gd.shape == wd.shape
    assert np.array_equal(gr, wr), np.argwhere(gr != wr)[:10]
    assert same_floats(gd, wd)


def names_of(V):
    return [b"w%d" % i for i in range(V)]


def questions(rng, V, Q):
    """random questions, the first eighth with b1 == b2 == b3"""
    b = rng.integers(0, V, (3, Q)).astype(np.int32)
    b[:, :max(1, Q // 8)] = b[0, :max(1, Q // 8)]
    return b


# D = 1250 is above the 1216 columns that a wavefront keeps in registers (the chunked walk over K)
@pytest.mark.parametrize("D", [1, 31, 32, 33, 65, 200, 400, 1000, 1250])
@pytest.mark.parametrize("V,Q", [(1, 1), (31, 33), (300, 300), (4133, 33)])
def test_top1_topk_equal_the_truth(gpu, D, V, Q, tmp_path):
    rng = np.random.default_rng(D * 10007 + V)
    T = make_codes(rng, "corr" if D % 2 == 0 else "random", V, D)
    path = write_packed_file(str(tmp_path / "v.w2bp"), names_of(V), pack_codes(T), D)
    ev = w2b.Evaluator(path, codes=True)
    assert ev.is_codes and not ev.is_bits and (ev.words, ev.size) == (V, D)
    b = questions(rng, V, Q)
    S = scores(T, *b)
    r1, d1 = ev.top1(*b)
    check((r1, d1), tuple(x[:, 0] for x in truth_from_scores(S, *b, 1)))
    for k in (1, 10, 64):
        got = ev.topk(*b, k)
        check(got, truth_from_scores(S, *b, k))
        if k == 1:
            check((got[0][:, 0], got[1][:, 0]), (r1, d1))
    ev.close()


# A workgroup walks several question tiles only when there are more tiles than the launch has ranges of them (about
# 1024 / row groups): 79 tiles against 61 (D = 65: the K loop has padding steps; D = 200: none) and 32 (D = 1250: chunked).
@pytest.mark.parametrize("D", [65, 200, 1250])
def test_many_question_tiles_per_workgroup(gpu, D, tmp_path):
    V, Q = 4133, 2500
    rng = np.random.default_rng(D + 5)
    T = make_codes(rng, "corr", V, D)
    path = write_packed_file(str(tmp_path / "v.w2bp"), names_of(V), pack_codes(T), D)
    ev = w2b.Evaluator(path, codes=True)
    b = questions(rng, V, Q)
    S = scores(T, *b)
    r1, d1 = ev.top1(*b)
    check((r1, d1), tuple(x[:, 0] for x in truth_from_scores(S, *b, 1)))
    for k in (1, 10, 64):
        check(ev.topk(*b, k), truth_from_scores(S, *b, k))
    ev.close()


def test_ties_exclusions_and_empty_lists(gpu, tmp_path):
    rng = np.random.default_rng(3)
    V, D = 700, 200
    T = make_codes(rng, "random", V, D)
    T[[5, 40, 41, 333, 650]] = T[9]              # duplicates of row 9: equal scores resolve to the lowest row
    T[V - 1] = -T[2]
    path = write_packed_file(str(tmp_path / "v.w2bp"), names_of(V), pack_codes(T), D)
    ev = w2b.Evaluator(path, codes=True)
    # the best rows (the duplicates of b2) are excluded ones: b1 / b3 are duplicates of b2
    b = np.array([[5, 40, 9, 100], [9, 9, 9, 9], [40, 5, 9, 333]], np.int32)
    check(ev.top1(*b), tuple(x[:, 0] for x in truth_topk(T, *b, 1)))
    for k in (3, 10, 64):
        check(ev.topk(*b, k), truth_topk(T, *b, k))
    rk, dk = ev.topk(*b, 10)
    assert rk[2, 0] == 5 and list(rk[2, :5]) == [5, 40, 41, 333, 650] and np.all(dk[2, :5] == dk[2, 0])
    rows = rng.integers(0, V, 40).astype(np.int32)
    got = ev.neighbors(rows, 10)
    check(got, truth_topk(T, rows, rows, rows, 10))
    check(got, ev.topk(rows, rows, rows, 10))
    # vec = -3 T[2] / |T[2]|: only rows that disagree with row 2 score above 0, fewer than k of them
    bn = np.array([[2], [V - 1], [V - 1]], np.int32)
    want = truth_topk(T, *bn, 64)
    check(ev.topk(*bn, 64), want)
    ev.close()
    # every row but the question's own is the opposite of the query: no answer
    base = make_codes(rng, "random", 1, 70)[0]
    N = np.tile(-base, (40, 1)).astype(np.int8)
    N[0] = N[1] = N[2] = base
    path = write_packed_file(str(tmp_path / "n.w2bp"), names_of(40), pack_codes(N), 70)
    ev = w2b.Evaluator(path, codes=True)
    b = np.array([[0], [1], [2]], np.int32)
    r, d = ev.top1(*b)
    assert r[0] == -1 and d.view(np.uint32)[0] == 0
    rk, dk = ev.topk(*b, 5)
    assert np.all(rk == -1) and np.all(dk.view(np.uint32) == 0)
    ev.close()


def test_threshold_scratch_budget_timing_and_argument_errors(gpu, tmp_path):
    rng = np.random.default_rng(9)
    V, D, Q, k = 3000, 200, 700, 10
    T = make_codes(rng, "corr", V, D)
    path = write_packed_file(str(tmp_path / "v.w2bp"), names_of(V), pack_codes(T), D)
    thr = 1234
    ev = w2b.Evaluator(path, threshold=thr, codes=True)
    assert ev.words == thr
    b = rng.integers(0, thr, (3, Q)).astype(np.int32)
    check(ev.topk(*b, k), truth_topk(T[:thr], *b, k))
    ev.close()
    ev = w2b.Evaluator(path, codes=True)
    b = rng.integers(0, V, (3, Q)).astype(np.int32)
    want = truth_topk(T, *b, k)
    ev.timing()
    check(ev.topk(*b, k), want)
    ms, launches, macs = ev.timing()
    assert launches == 1 and ms > 0 and macs == 3.0 * Q * V * D
    ev.set_topk_scratch(1)                                   # one 128-question chunk per launch
    check(ev.topk(*b, k), want)
    assert ev.timing()[1] == (Q + 127) // 128
    ev.set_topk_scratch(300 * 8 * 3000)                      # a mid value: a few chunks
    check(ev.topk(*b, k), want)
    ev.set_topk_scratch(0)
    ev.set_kernel(0)                                         # accepted, nothing to select
    check(ev.topk(*b, k), want)
    for bad_k in (0, 65):
        with pytest.raises(w2b.W2bError):
            ev.topk(*b, bad_k)
    b[1, 3] = V
    with pytest.raises(w2b.W2bError):
        ev.top1(*b)
    for f in (ev.matrix, ev.bits):
        with pytest.raises(w2b.W2bError) as e:
            f()
        assert e.value.code == _lib.W2B_EINVAL
    ev.close()


def test_loading_packed_and_float_files(gpu, tmp_path):
    rng = np.random.default_rng(21)
    V, D = 300, 130
    T = make_codes(rng, "random", V, D)
    pk = write_packed_file(str(tmp_path / "m.w2bp"), names_of(V), pack_codes(T), D)
    fl = write_vectors_file(str(tmp_path / "m.bin"), names_of(V), values_of(T))
    a, b = w2b.Evaluator(pk, codes=True), w2b.Evaluator(fl, codes=True)
    assert np.array_equal(a.codes(), pack_codes(T)) and np.array_equal(b.codes(), a.codes())
    assert [a.word(i) for i in range(V)] == [b.word(i) for i in range(V)] == [n.upper() for n in names_of(V)]
    q = rng.integers(0, V, (3, 50)).astype(np.int32)
    check(a.topk(*q, 7), b.topk(*q, 7))
    a.close(); b.close()
    # any float file: negative iff num < 0, .25 iff |num| <= .5 -- NaN is +.75, +0 and -0 are +.25
    X = rng.standard_normal((V, D)).astype(np.float32)
    X[:, 3], X[:, 64], X[:, 129] = 0.0, -0.0, np.nan
    X[5, 7], X[6, 8], X[7, 9], X[8, 10] = -np.inf, np.inf, 0.5, -0.5
    fx = write_vectors_file(str(tmp_path / "x.bin"), names_of(V), X)
    c = w2b.Evaluator(fx, threshold=200, codes=True)
    with np.errstate(invalid="ignore"):
        Tx = (np.where(X < 0, -1, 1) * np.where(np.abs(X) <= 0.5, 1, 3)).astype(np.int8)
    assert np.all(Tx[:, [3, 64]] == 1) and np.all(Tx[:, 129] == 3) and c.words == 200
    assert (Tx[5, 7], Tx[6, 8], Tx[7, 9], Tx[8, 10]) == (-3, 3, 1, -1)
    assert np.array_equal(codes_of_packed(c.codes(), D), Tx[:200])
    c.close()
    one = write_packed_file_1bit(str(tmp_path / "one.w2bp"), names_of(4), pack_signs(make_signs(rng, "random", 4, 9)), 9)
    with pytest.raises(w2b.W2bError) as e:
        w2b.Evaluator(one, codes=True)
    assert e.value.code == _lib.W2B_EINVAL and "bits" in str(e.value)
    with pytest.raises(w2b.W2bError) as e:
        w2b.Evaluator(str(tmp_path / "missing.w2bp"), codes=True)
    assert e.value.code == _lib.W2B_EIO and "Input file not found" in str(e.value)
    f32 = w2b.Evaluator(fl)
    assert not f32.is_codes
    with pytest.raises(w2b.W2bError) as e:
        f32.codes()
    assert e.value.code == _lib.W2B_EINVAL
    f32.close()


def small_trainer(tmp_path, bitlevel, rng):
    V, D = 90, 70
    words = ["</s>"] + ["w%d" % i for i in range(1, V)]
    words[5] = "x" * 57
    words[40] = "Mixed_Case"
    corpus = str(tmp_path / ("c%d.txt" % bitlevel))
    toks = rng.integers(1, V, 6000)
    with open(corpus, "wb") as f:
        for i in range(0, len(toks), 20):
            f.write(" ".join(words[t] for t in toks[i:i + 20]).encode("latin1") + b"\n")
    c = w2b.Corpus(corpus, 1)
    t = w2b.Trainer(c.vocab_size, D, 5, 5, bitlevel, num_threads=4, iter=1, sample=0.0, train_words=c.train_words)
    t.init_net()
    t.set_vocab_counts(c.counts(), 100000)
    t.set_corpus(c.tokens())
    starts, ov = c.shards(4)
    t.set_shards(starts, ov)
    t.train_epoch(500)
    return c, t, D


def test_from_trainer_equals_the_saved_packed_file(gpu, tmp_path):
    rng = np.random.default_rng(8)
    c, t, D = small_trainer(tmp_path, 2, rng)
    pk = str(tmp_path / "v.w2bp")
    c.save_vectors_packed(pk, t.export_packed(), D, 2)
    a = w2b.Evaluator(pk, codes=True)
    b = w2b.Evaluator.from_trainer(t, c.words(), codes=True)
    cut = w2b.Evaluator.from_trainer(t, c.words(), threshold=37, codes=True)
    try:
        assert b.is_codes and (a.words, a.size) == (b.words, b.size) and cut.words == 37
        assert [a.word(i) for i in range(a.words)] == [b.word(i) for i in range(b.words)]
        assert np.array_equal(a.codes(), b.codes()) and np.array_equal(cut.codes(), a.codes()[:37])
        assert np.array_equal(a.codes(), w2b.pack_quantized(t.export_quantized(), 2))
        q = rng.integers(0, a.words, (3, 200)).astype(np.int32)
        check(a.topk(*q, 10), b.topk(*q, 10))
        check(a.top1(*q), b.top1(*q))
        check(b.topk(*q, 10), truth_topk(codes_of_packed(a.codes(), D), *q, 10))
        qs = (": s\n" + "".join("%s %s %s %s\n" % tuple(c.words()[j] for j in rng.integers(1, c.vocab_size, 4))
                                for _ in range(300))).encode("latin1")
        assert a.transcript(qs) == b.transcript(qs)
    finally:
        a.close(); b.close(); cut.close(); t.close(); c.close()
    c1, t1, _ = small_trainer(tmp_path, 1, rng)
    try:
        with pytest.raises(w2b.W2bError) as e:
            w2b.Evaluator.from_trainer(t1, c1.words(), codes=True)
        assert e.value.code == _lib.W2B_EINVAL
    finally:
        t1.close(); c1.close()


def test_transcript_and_command_lines(gpu, tmp_path):
    """On a model whose every best row leads its runner-up by more than twice the bound between the fp32 path and the codes
    path (asserted on the truth), the codes transcript is the fp32 fused transcript, byte for byte -- also through
    ./compute_accuracy ... codes; ./nearest ... codes equals nearest_text."""
    E = eval_oracle()
    rng = np.random.default_rng(12)
    V, D, Q = 500, 100, 120
    T = make_codes(rng, "random", V, D)
    names = names_of(V)
    fl = write_vectors_file(str(tmp_path / "m.bin"), names, values_of(T))
    pk = write_packed_file(str(tmp_path / "m.w2bp"), names, pack_codes(T), D)
    b = rng.integers(0, V, (4, Q))
    b[:, -1] = (1, 2, 3, 4)
    assert lead_over_runner_up(scores(T, *b[:3]), *b[:3]).min() > 2 * float_bound(D)
    qs = (b": capital\n" + b"".join(b"w%d w%d w%d w%d\n" % tuple(b[:, q]) for q in range(Q - 1)) +
          b"nope w1 w2 w3\n: gram1\nw1 w2 w3 w4\n")
    f32 = w2b.Evaluator(fl, 2, 0, fused=True)
    want = f32.transcript(qs)
    f32.close()
    ev = w2b.Evaluator(pk, codes=True)
    assert ev.transcript(qs) == want
    om = E.EvalModel(fl, 2, 0)
    assert E.transcript(TruthModel(om, T), qs) == want
    r = subprocess.run([ACC, pk, "0", "0", "codes"], input=qs, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    queries = b"w7\nw1 w2  w3\nw4 w5\nno-such-word\n"
    text = ev.nearest_text(queries, 10)
    rows, sc = truth_topk(T, [7], [7], [7], 10)
    first = b"W7:\n" + b"".join(b"%d\tW%d\t%s\n" % (j + 1, rows[0, j], ("%.6f" % float(sc[0, j])).encode())
                               for j in range(10) if rows[0, j] >= 0)
    assert text.startswith(first) and b": expected 1 or 3 words\n" in text and b": not in vocabulary: NO-SUCH-WORD\n" in text
    r = subprocess.run([NEAR, pk, "10", "0", "0", "codes"], input=queries, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == text, r.stderr
    ev.close()


def test_word2bits_eval_bits_at_bitlevel_2(gpu, tmp_path):
    """./word2bits -bitlevel 2 -eval Q -eval-bits 1 (a fresh child process) prints the transcript that the codes evaluator
    gives on the packed file the same run saved.  That is the wiring: nothing guarantees that every best row of a freshly
    trained model leads its runner-up by more than twice the bound, so the comparison with the fp32 fused transcript is
    made on the seeded model of test_transcript_and_command_lines, through the same evaluator entry points."""
    rng = np.random.default_rng(4)
    V = 60
    corpus = str(tmp_path / "c.txt")
    toks = rng.integers(1, V, 8000)
    with open(corpus, "wb") as f:
        for i in range(0, len(toks), 20):
            f.write(" ".join("w%d" % t for t in toks[i:i + 20]).encode() + b"\n")
    qfile = str(tmp_path / "q.txt")
    with open(qfile, "wb") as f:
        f.write(b": s\n" + b"".join(b"w%d w%d w%d w%d\n" % tuple(rng.integers(1, V, 4)) for _ in range(100)))
    out, pk = str(tmp_path / "v.bin"), str(tmp_path / "v.w2bp")
    r = subprocess.run([W2B, "-train", corpus, "-output", out, "-size", "40", "-bitlevel", "2", "-binary", "1", "-min-count", "1",
                        "-threads", "2", "-iter", "1", "-packed", pk, "-eval", qfile, "-eval-bits", "1"],
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ev = w2b.Evaluator(pk, codes=True)
    want = ev.transcript(open(qfile, "rb").read())
    ev.close()
    assert want in r.stdout and b"ACCURACY TOP1" in want


def test_two_hundred_thousand_rows_stay_packed(gpu, tmp_path):
    """V = 200 000, D = 400 from a .w2bp written here: 22.4 MB of packed rows (a float matrix would be 320 MB).  The
    handle plus a 6-question top-1 / top-10 / top-64 stays below 2 x packed bytes + 64 MiB (the bits test's allowance);
    results against the truth computed in row blocks."""
    import torch
    V, D = 200_000, 400
    rng = np.random.default_rng(77)
    nb = (D + 63) // 64
    packed = rng.integers(0, 2 ** 64, (V, 2 * nb), dtype=np.uint64)
    packed[:, -2:] &= np.uint64((1 << (D - 64 * (nb - 1))) - 1)       # padding bits are zero in the file
    src = np.array([10, 100_000, 199_999, 123_456], np.int64)
    for j, s in enumerate(src):                               # near copies of four rows, far apart in the file
        for t in range(5):
            row = packed[s].copy()
            row[2 * (t % nb)] ^= np.uint64(0xFF << (3 * j))
            packed[(s + 7919 * (t + 1) * (j + 1)) % V] = row
    with open(str(tmp_path / "big.w2bp"), "wb") as f:
        f.write(b"W2BP1 %d %d 2\n" % (V, D))
        f.write(b"".join(b"w%d\n" % i for i in range(V)))
        f.write(packed.astype("<u8").tobytes())
    free0 = torch.cuda.mem_get_info()[0]
    ev = w2b.Evaluator(str(tmp_path / "big.w2bp"), codes=True)
    b = np.array([[10, 100_000, 199_999, 123_456, 5, 77],
                  [10, 100_000, 199_999, 123_456, 6, 10],
                  [10, 100_000, 199_999, 123_456, 7, 100_000]], np.int32)
    got1, got10, got64 = ev.top1(*b), ev.topk(*b, 10), ev.topk(*b, 64)
    used = free0 - torch.cuda.mem_get_info()[0]
    print("device footprint %.1f MiB for %.1f MiB of packed rows" % (used / 2 ** 20, packed.nbytes / 2 ** 20))
    assert used < 2 * packed.nbytes + (64 << 20)
    assert np.array_equal(ev.codes()[::9973], packed[::9973])
    S = scores(codes_of_packed(packed, D), *b)                # (the products go through the rows in blocks of 65536)
    check(got1, tuple(x[:, 0] for x in truth_from_scores(S, *b, 1)))
    check(got10, truth_from_scores(S, *b, 10))
    check(got64, truth_from_scores(S, *b, 64))
    assert np.all(got10[0][:4, :5] >= 0) and np.all(got10[1][:4, :5] > 0.9)     # the planted near copies lead
    ev.close()
