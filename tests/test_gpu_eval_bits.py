"""Bits-mode evaluator on the GPU (include/word2bits_eval.h, "bits mode"): rows and score bits exactly equal to the numpy
implementation of the stated semantics (bits_testlib), which tests/test_eval_bits_host.py ties to the pinned float
oracle; no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import GOLDEN, ROOT, eval_oracle, write_vectors_file
from topk_testlib import same_floats
from bits_testlib import (THIRD, TruthModel, int_scores, make_signs, pack_signs, signs_of_bits, truth_from_scores,
                          truth_top1, truth_topk, values_of, write_packed_file)

pytestmark = pytest.mark.gpu
ACC, NEAR = os.path.join(ROOT, "compute_accuracy"), os.path.join(ROOT, "nearest")


def check(got, want):
    (gr, gd), (wr, wd) = got, want
    assert gr.shape == wr.shape and gd.shape == wd.shape
    assert np.array_equal(gr, wr), np.argwhere(gr != wr)[:10]
    assert same_floats(gd, wd)


def names_of(V):
    return [b"w%d" % i for i in range(V)]


def questions(rng, S, Q):
    """random questions, the first eighth with b1 == b2 == b3"""
    V = S.shape[0]
    b = rng.integers(0, V, (3, Q)).astype(np.int32)
    b[:, :max(1, Q // 8)] = b[0, :max(1, Q // 8)]
    return b


@pytest.mark.parametrize("kind", ["random", "corr"])
@pytest.mark.parametrize("D", [1, 7, 37, 63, 64, 65, 200, 300, 1000])
@pytest.mark.parametrize("V", [1, 5, 127, 128, 129, 3000])
def test_top1_topk_neighbors_equal_the_truth(gpu, kind, D, V, tmp_path):
    rng = np.random.default_rng(D * 10007 + V)
    S = make_signs(rng, kind, V, D)
    if V >= 127:
        S[V - 3] = -S[2]                                     # a row nothing agrees with: questions without an answer
    path = write_packed_file(str(tmp_path / "v.w2bp"), names_of(V), pack_signs(S), D)
    ev = w2b.Evaluator(path, bits=True)
    assert ev.is_bits and (ev.words, ev.size) == (V, D)
    Q = 200 if V >= 127 else 24
    b = questions(rng, S, Q)
    I = int_scores(S, *b)
    r1, d1 = ev.top1(*b)
    check((r1, d1), tuple(x[:, 0] for x in truth_from_scores(I, *b, 1, D)))
    for k in (1, 2, 10, 64):
        got = ev.topk(*b, k)
        check(got, truth_from_scores(I, *b, k, D))
        if k == 1:                                           # k = 1 equals top1
            check((got[0][:, 0], got[1][:, 0]), (r1, d1))
    rows = b[0]
    got = ev.neighbors(rows, 10)
    check(got, truth_topk(S, rows, rows, rows, 10))
    check(got, ev.topk(rows, rows, rows, 10))
    if V == 1:
        assert np.all(ev.topk(*b, 2)[0] == -1)               # the only row is the question's own
    if V >= 127:
        bn = np.array([[2], [V - 3], [V - 3]], np.int32)     # vec = -3 S[2]: only rows that disagree with row 2 score above 0
        check(ev.top1(*bn), truth_top1(S, *bn))
    if V == 3000 and kind == "corr":
        tied = ev.topk(*b, 10)[1]
        assert np.any((tied[:, 1:] == tied[:, :-1]) & (tied[:, 1:] > 0))          # ties inside the lists
    ev.close()


def test_questions_without_an_answer_give_row_minus_one(gpu, tmp_path):
    """best I <= 0: every row but the three of the question is the exact opposite of the query"""
    D, V = 70, 40
    rng = np.random.default_rng(4)
    base = make_signs(rng, "random", 1, D)[0]
    S = np.tile(-base, (V, 1)).astype(np.int8)
    S[0] = S[1] = S[2] = base
    S[3, :D // 2] = base[:D // 2]                            # I == 0 exactly (D even): never an answer
    path = write_packed_file(str(tmp_path / "v.w2bp"), names_of(V), pack_signs(S), D)
    ev = w2b.Evaluator(path, bits=True)
    b = np.array([[0], [1], [2]], np.int32)
    assert int_scores(S, *b)[0, 3] == 0 and int_scores(S, *b)[0, 4:].max() < 0
    r, d = ev.top1(*b)
    assert r[0] == -1 and d[0] == 0 and d.view(np.uint32)[0] == 0
    rk, dk = ev.topk(*b, 5)
    assert np.all(rk == -1) and np.all(dk.view(np.uint32) == 0)
    ev.close()


def test_threshold_scratch_budget_and_argument_errors(gpu, tmp_path):
    rng = np.random.default_rng(9)
    V, D, Q, k = 3000, 200, 700, 10
    S = make_signs(rng, "corr", V, D)
    path = write_packed_file(str(tmp_path / "v.w2bp"), names_of(V), pack_signs(S), D)
    thr = 1234
    ev = w2b.Evaluator(path, threshold=thr, bits=True)
    assert ev.words == thr
    b = rng.integers(0, thr, (3, Q)).astype(np.int32)
    check(ev.topk(*b, k), truth_topk(S[:thr], *b, k))
    ev.close()
    ev = w2b.Evaluator(path, bits=True)
    b = rng.integers(0, V, (3, Q)).astype(np.int32)
    want = truth_topk(S, *b, k)
    ev.timing()
    check(ev.topk(*b, k), want)
    ms, launches, macs = ev.timing()
    assert launches == 1 and ms > 0 and macs == 1.0 * Q * V * D
    ev.set_topk_scratch(1)                                   # one 128-question chunk per launch, one row range
    check(ev.topk(*b, k), want)
    assert ev.timing()[1] == (Q + 127) // 128
    ev.set_topk_scratch(128 * 8 * k * 4)                     # room for three row ranges of 128 questions
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
    with pytest.raises(w2b.W2bError) as e:
        ev.matrix()
    assert e.value.code == _lib.W2B_EINVAL
    ev.close()


def test_one_million_rows_stay_packed(gpu, tmp_path):
    """V = 1 000 000, D = 1000 from a .w2bp written here: results against the truth (numpy works through the rows in
    blocks of 65536, a few seconds per question batch), and the evaluator's device footprint.  The packed rows are
    128 MB; a [V][D] float matrix would be 4 GB.  Allowance: 64 MiB for the allocator's granularity, the stream and the
    questions' scratch (planes, keys and the top-k slots of 6 questions over 1024 row ranges: about 3 MiB)."""
    import torch
    V, D, Q = 1_000_000, 1000, 6
    rng = np.random.default_rng(77)
    wpr = (D + 63) // 64
    packed = rng.integers(0, 2 ** 64, (V, wpr), dtype=np.uint64)
    packed[:, -1] &= np.uint64((1 << (D - 64 * (wpr - 1))) - 1)       # padding bits are zero in the file
    src = np.array([10, 500_000, 999_999, 123_456], np.int64)
    for j, s in enumerate(src):                               # near copies of four rows, far apart in the file
        for t in range(5):
            row = packed[s].copy()
            row[t] ^= np.uint64(0xFF << (3 * j))
            packed[(s + 7919 * (t + 1) * (j + 1)) % V] = row
    with open(str(tmp_path / "big.w2bp"), "wb") as f:
        f.write(b"W2BP1 %d %d 1\n" % (V, D))
        f.write(b"".join(b"w%d\n" % i for i in range(V)))
        f.write(packed.astype("<u8").tobytes())
    free0 = torch.cuda.mem_get_info()[0]
    ev = w2b.Evaluator(str(tmp_path / "big.w2bp"), bits=True)
    b = np.array([[10, 500_000, 999_999, 123_456, 5, 77],
                  [10, 500_000, 999_999, 123_456, 6, 10],
                  [10, 500_000, 999_999, 123_456, 7, 500_000]], np.int32)
    got1, got10, got64 = ev.top1(*b), ev.topk(*b, 10), ev.topk(*b, 64)
    used = free0 - torch.cuda.mem_get_info()[0]
    print("device footprint %.1f MiB for %.1f MiB of packed rows" % (used / 2 ** 20, packed.nbytes / 2 ** 20))
    assert used < 2 * packed.nbytes + (64 << 20)
    assert np.array_equal(ev.bits()[::9973], packed[::9973])
    S = signs_of_bits(packed, D)
    del packed
    I = int_scores(S, *b.astype(np.int64))
    check(got1, tuple(x[:, 0] for x in truth_from_scores(I, *b, 1, D)))
    check(got10, truth_from_scores(I, *b, 10, D))
    check(got64, truth_from_scores(I, *b, 64, D))
    assert np.all(got10[0][:4, :5] >= 0) and np.all(got10[1][:4, :5] > 0.9)     # the planted near copies lead
    ev.close()


def test_loading_packed_and_float_files(gpu, tmp_path):
    rng = np.random.default_rng(21)
    V, D = 300, 130
    S = make_signs(rng, "random", V, D)
    vals = values_of(S)
    pk = write_packed_file(str(tmp_path / "m.w2bp"), names_of(V), pack_signs(S), D)
    fl = write_vectors_file(str(tmp_path / "m.bin"), names_of(V), vals)
    a, b = w2b.Evaluator(pk, bits=True), w2b.Evaluator(fl, bits=True)
    assert np.array_equal(a.bits(), pack_signs(S)) and np.array_equal(b.bits(), a.bits())
    assert [a.word(i) for i in range(V)] == [b.word(i) for i in range(V)] == [n.upper() for n in names_of(V)]
    q = rng.integers(0, V, (3, 50)).astype(np.int32)
    check(a.topk(*q, 7), b.topk(*q, 7))
    a.close(); b.close()
    # any float file: negative iff num < 0 -- +0, -0 and NaN are positive, as quantize(x, 1) has them
    X = rng.standard_normal((V, D)).astype(np.float32)
    X[:, 3], X[:, 64], X[:, 129] = 0.0, -0.0, np.nan
    X[5, 7], X[6, 8] = -np.inf, np.inf
    fx = write_vectors_file(str(tmp_path / "x.bin"), names_of(V), X)
    c = w2b.Evaluator(fx, threshold=200, bits=True)
    Sx = np.where(X < 0, -1, 1).astype(np.int8)
    assert np.all(Sx[:, [3, 64, 129]] == 1) and c.words == 200
    assert np.array_equal(c.bits(), pack_signs(Sx[:200]))
    c.close()
    two = str(tmp_path / "two.w2bp")
    with open(two, "wb") as f:
        f.write(b"W2BP1 2 5 2\na\nb\n" + np.zeros(4, "<u8").tobytes())
    with pytest.raises(w2b.W2bError) as e:
        w2b.Evaluator(two, bits=True)
    assert e.value.code == _lib.W2B_EINVAL
    with pytest.raises(w2b.W2bError) as e:
        w2b.Evaluator(str(tmp_path / "missing.w2bp"), bits=True)
    assert e.value.code == _lib.W2B_EIO and "Input file not found" in str(e.value)
    f32 = w2b.Evaluator(fl)
    assert not f32.is_bits
    with pytest.raises(w2b.W2bError) as e:
        f32.bits()
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
    c, t, D = small_trainer(tmp_path, 1, rng)
    pk = str(tmp_path / "v.w2bp")
    c.save_vectors_packed(pk, t.export_packed(), D, 1)
    a = w2b.Evaluator(pk, bits=True)
    b = w2b.Evaluator.from_trainer(t, c.words(), bits=True)
    cut = w2b.Evaluator.from_trainer(t, c.words(), threshold=37, bits=True)
    try:
        assert b.is_bits and (a.words, a.size) == (b.words, b.size) and cut.words == 37
        assert [a.word(i) for i in range(a.words)] == [b.word(i) for i in range(b.words)]
        assert np.array_equal(a.bits(), b.bits()) and np.array_equal(cut.bits(), a.bits()[:37])
        assert np.array_equal(a.bits(), w2b.pack_quantized(t.export_quantized(), 1))
        q = rng.integers(0, a.words, (3, 200)).astype(np.int32)
        check(a.topk(*q, 10), b.topk(*q, 10))
        check(a.top1(*q), b.top1(*q))
        check(b.topk(*q, 10), truth_topk(signs_of_bits(a.bits(), D), *q, 10))
        qs = (": s\n" + "".join("%s %s %s %s\n" % tuple(c.words()[j] for j in rng.integers(1, c.vocab_size, 4))
                                for _ in range(300))).encode("latin1")
        assert a.transcript(qs) == b.transcript(qs)
    finally:
        a.close(); b.close(); cut.close(); t.close(); c.close()
    c2, t2, _ = small_trainer(tmp_path, 2, rng)
    try:
        with pytest.raises(w2b.W2bError) as e:
            w2b.Evaluator.from_trainer(t2, c2.words(), bits=True)
        assert e.value.code == _lib.W2B_EINVAL
    finally:
        t2.close(); c2.close()


def float_and_bits_agree(fl_path, S, b):
    """the float path's answers have the bits path's integer scores; only the choice of rows among ties may differ"""
    D = S.shape[1]
    I = int_scores(S, *b)
    for fused in (True, False):
        f = w2b.Evaluator(fl_path, 0, 0, fused=fused)
        fr1, _ = f.top1(*b)
        fr10, _ = f.topk(*b, 10)
        f.close()
        e = w2b.Evaluator(fl_path, bits=True)
        br1, _ = e.top1(*b)
        br10, _ = e.topk(*b, 10)
        e.close()
        answered = 0
        for q in range(b.shape[1]):
            if br1[q] >= 0:
                assert fr1[q] >= 0 and I[q, fr1[q]] == I[q, br1[q]], (fused, q)
                answered += 1
            fi = [I[q, r] for r in fr10[q] if r >= 0 and I[q, r] > 0]      # (the float list may end in rows with I == 0)
            bi = [I[q, r] for r in br10[q] if r >= 0]
            assert fi == bi, (fused, q, fi, bi)
        assert answered > b.shape[1] // 2


def test_agreement_with_the_float_path_on_the_gpu(gpu, tmp_path):
    E = eval_oracle()
    fix = os.path.join(GOLDEN, "eval_1bit.bin")
    om = E.EvalModel(fix, 0, 0)
    tm = TruthModel(om)
    rng = np.random.default_rng(31)
    b = rng.integers(0, om.words, (3, 500)).astype(np.int32)
    float_and_bits_agree(fix, tm.S, b)
    V, D = 3000, 200
    S = make_signs(rng, "corr", V, D)
    fl = write_vectors_file(str(tmp_path / "s.bin"), names_of(V), values_of(S))
    b = rng.integers(0, V, (3, 500)).astype(np.int32)
    b[:, :40] = b[0, :40]
    float_and_bits_agree(fl, S, b)


def test_transcript_and_command_lines(gpu, tmp_path):
    """w2b_eval_transcript on a bits handle is the oracle's transcript() over a model whose top1 is the numpy truth;
    ./compute_accuracy ... bits prints the same bytes; ./nearest ... bits equals nearest_text"""
    E = eval_oracle()
    fix = os.path.join(GOLDEN, "eval_1bit.bin")
    om = E.EvalModel(fix, 0, 0)
    tm = TruthModel(om)
    raw = np.where(om.M < 0, -THIRD, THIRD).astype(np.float32)
    pk = str(tmp_path / "f.w2bp")
    with open(fix, "rb") as f:                               # the fixture's own names, as its file spells them
        data = f.read()
    pos = data.index(b"\n") + 1
    names = []
    for _ in range(om.words):
        sp = data.index(b" ", pos)
        names.append(data[pos:sp])
        pos = sp + 1 + 4 * om.size + 1
    if any(b"\n" in n for n in names):
        pytest.fail("the 1-bit fixture's names were expected to be plain words")
    write_packed_file(pk, names, w2b.pack_quantized(raw, 1), om.size)
    ev, evf = w2b.Evaluator(pk, bits=True), w2b.Evaluator(fix, bits=True)
    assert np.array_equal(ev.bits(), evf.bits())
    for qn in ("eval_q_1bit.txt", "eval_q_noeol.txt", "eval_q_empty.txt"):
        qs = open(os.path.join(GOLDEN, qn), "rb").read()
        want = E.transcript(tm, qs)
        assert ev.transcript(qs) == want and evf.transcript(qs) == want, qn
        r = subprocess.run([ACC, pk, "0", "0", "bits"], input=qs, capture_output=True, timeout=300)
        assert r.returncode == 0 and r.stdout == want, (qn, r.stderr)
    assert b"ACCURACY TOP1" in E.transcript(tm, open(os.path.join(GOLDEN, "eval_q_1bit.txt"), "rb").read())
    known = [n for n in om.names if n and om.lookup(n) < om.words][1:8]
    queries = b"\n".join([known[0].lower(), known[1] + b" " + known[2] + b"  " + known[3], known[4] + b" " + known[5],
                          b"no-such-word", known[6]]) + b"\n"
    text = ev.nearest_text(queries, 10)
    r0 = om.lookup(known[0])
    rows, scores = truth_topk(tm.S, [r0], [r0], [r0], 10)
    first = known[0] + b":\n" + b"".join(b"%d\t%s\t%s\n" % (j + 1, om.names[rows[0, j]], ("%.6f" % float(scores[0, j])).encode())
                                        for j in range(10) if rows[0, j] >= 0)
    assert text.startswith(first) and b": expected 1 or 3 words\n" in text and b": not in vocabulary: NO-SUCH-WORD\n" in text
    r = subprocess.run([NEAR, pk, "10", "0", "0", "bits"], input=queries, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == text, r.stderr
    ev.close(); evf.close()
