"""Top-k neighbour and analogy queries (ref src/compute-accuracy.c:155-177 with N = k) on the GPU: rows and score bits
against the pinned oracle (topk_testlib.oracle_topk: k rounds of its top-1), no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from w2b_testlib import GOLDEN, ROOT, eval_oracle, read_vectors, write_vectors_file
from topk_testlib import oracle_topk, same_floats, seeded_matrix

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "nearest")


def check(got, want):
    (gr, gd), (wr, wd) = got, want
    assert gr.shape == wr.shape and gd.shape == wd.shape
    assert np.array_equal(gr, wr), np.argwhere(gr != wr)[:10]
    assert same_floats(gd, wd)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("vec,bitlevel,threshold", [("eval_1bit.bin", 0, 0), ("eval_1bit.bin", 0, 100),
                                                    ("eval_fp.bin", 0, 0), ("eval_fp.bin", 1, 0),
                                                    ("eval_fp.bin", 2, 0), ("eval_fp.bin", 4, 0),
                                                    ("eval_fp.bin", 3, 150), ("eval_fp.bin", 8, 0)])
def test_topk_bit_exact_on_fixtures(gpu, vec, bitlevel, threshold, fused):
    E = eval_oracle()
    path = os.path.join(GOLDEN, vec)
    om = E.EvalModel(path, bitlevel, threshold, fma=fused)
    ev = w2b.Evaluator(path, bitlevel, threshold, fused=fused)
    rng = np.random.default_rng(5)
    b = rng.integers(0, ev.words, (3, 400)).astype(np.int32)
    b[:, :20] = b[0, :20]                      # b1 == b2 == b3
    for k in (1, 5, 64):
        check(ev.topk(*b, k), oracle_topk(om, *b, k))
    r1, d1 = ev.topk(*b, 1)
    t1, td1 = ev.top1(*b)
    assert np.array_equal(r1[:, 0], t1) and np.array_equal(d1[:, 0].view(np.uint32), td1.view(np.uint32))
    ev.close()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kind,V,D,Q,k", [("1bit", 3000, 200, 300, 10), ("1bit", 3000, 200, 130, 64),
                                          ("2bit", 1500, 400, 200, 10), ("2bit", 1500, 400, 130, 64),
                                          ("fp", 5000, 300, 200, 10), ("fp", 5000, 300, 130, 64),
                                          ("fp", 777, 1000, 130, 10), ("fp", 777, 1000, 130, 64),
                                          ("1bit", 129, 5, 257, 64)])
def test_topk_bit_exact_on_seeded_inputs(gpu, kind, V, D, Q, k, fused, tmp_path):
    """sizes that cross tile edges, b1 == b2 == b3 questions, a zero (NaN) row; the 1-bit inputs tie inside the lists;
    129 x 5 is the short-list case (every list ends in -1 / 0)"""
    E = eval_oracle()
    rng = np.random.default_rng(V + D)
    M = seeded_matrix(rng, kind, V, D)
    M[V // 2] = 0                               # NaN after the normalisation
    path = write_vectors_file(str(tmp_path / "v.bin"), [b"w%d" % i for i in range(V)], M)
    om, ev = E.EvalModel(path, 0, 0, fma=fused), w2b.Evaluator(path, 0, 0, fused=fused)
    b = rng.integers(0, V, (3, Q)).astype(np.int32)
    b[:, :10] = b[0, :10]
    b[0, 10] = V // 2                           # a NaN query vector: nothing qualifies
    want = oracle_topk(om, *b, k)
    check(ev.topk(*b, k), want)
    if fused:                                   # the same fused chain on the vector ALU
        ev.set_kernel(0)
        check(ev.topk(*b, k), want)
        ev.set_kernel(1)
    if V == 129:
        short = want[0][:, -1] == -1               # about half of the 129 rows score above 0
        assert short.mean() >= 0.5 and np.all(want[1][short, -1] == 0)
    if (kind, V, k) == ("1bit", 3000, 10):      # really tie-heavy: equal scores inside the top 10
        d = want[1]
        tied = np.any((d[:, 1:] == d[:, :-1]) & (d[:, 1:] > 0), axis=1)
        assert tied.mean() >= 0.25, tied.mean()
    ev.close()


@pytest.mark.parametrize("fused", [True, False])
def test_neighbors_equal_topk_of_the_row(gpu, fused, tmp_path):
    E = eval_oracle()
    rng = np.random.default_rng(3)
    V, D = 1000, 70
    M = seeded_matrix(rng, "fp", V, D)
    M[::7] = np.abs(M[::7]) * 0                 # zero rows (NaN) among the queries as well
    M[5] = M[900]
    path = write_vectors_file(str(tmp_path / "v.bin"), [b"w%d" % i for i in range(V)], M)
    om, ev = E.EvalModel(path, 0, 0, fma=fused), w2b.Evaluator(path, 0, 0, fused=fused)
    rows = rng.integers(0, V, 300).astype(np.int32)
    rows[0] = 900
    got = ev.neighbors(rows, 7)
    check(got, ev.topk(rows, rows, rows, 7))
    check(got, oracle_topk(om, rows, rows, rows, 7))
    assert got[0][0, 0] == 5
    ev.close()


def test_results_do_not_depend_on_scratch_or_question_order(gpu, tmp_path):
    rng = np.random.default_rng(9)
    V, D, Q, k = 3000, 200, 700, 10
    M = seeded_matrix(rng, "1bit", V, D)
    path = write_vectors_file(str(tmp_path / "v.bin"), [b"w%d" % i for i in range(V)], M)
    ev = w2b.Evaluator(path, 0, 0)
    b = rng.integers(0, V, (3, Q)).astype(np.int32)
    ev.timing()
    base = ev.topk(*b, k)
    assert ev.timing()[1] == 1
    ev.set_topk_scratch(1)                      # one 128-question tile per launch
    check(ev.topk(*b, k), base)
    assert ev.timing()[1] == (Q + 127) // 128
    ev.set_topk_scratch(0)
    perm = rng.permutation(Q)
    r, d = ev.topk(*b[:, perm], k)
    check((r, d), (base[0][perm], base[1][perm]))
    with pytest.raises(w2b.W2bError):
        ev.topk(*b, 0)
    with pytest.raises(w2b.W2bError):
        ev.topk(*b, 65)
    b[1, 3] = V
    with pytest.raises(w2b.W2bError):
        ev.topk(*b, k)
    ev.close()


def test_full_size_properties(gpu, tmp_path):
    """text8-sized vocabulary (60238 x 200, 1-bit): three copies of each of 300 source rows planted at low row numbers
    are the source's three nearest rows, in ascending row order with bit-equal scores (|row|^2)."""
    V, D = 60238, 200
    rng = np.random.default_rng(11)
    M = (rng.integers(0, 2, (V, D)) * 2 - 1).astype(np.float32) / np.float32(3)
    src = rng.choice(np.arange(2000, V), 300, replace=False).astype(np.int32)
    for j in range(3):
        M[200 + 300 * j:500 + 300 * j] = M[src]
    path = write_vectors_file(str(tmp_path / "v.bin"), [b"w%d" % i for i in range(V)], M)
    ev = w2b.Evaluator(path, 0, 0)
    rows, d = ev.neighbors(src, 3)
    want = np.stack([200 + 300 * j + np.arange(300) for j in range(3)], 1).astype(np.int32)
    assert np.array_equal(rows, want)
    assert np.all(d > 0.99) and np.all(d < 1.01)
    assert np.all(d.view(np.uint32) == d.view(np.uint32)[:, :1])
    ev.timing()
    b = rng.integers(0, V, (3, 20000)).astype(np.int32)
    r, d = ev.topk(*b, 10)
    ms, launches, macs = ev.timing()
    assert launches >= 1 and ms > 0 and macs >= 1.0 * 20000 * V * D
    assert np.all(r >= 0) and np.all(d[:, :-1] >= d[:, 1:]) and np.all(d > 0)
    tie = d[:, :-1] == d[:, 1:]
    assert np.all(r[:, :-1][tie] < r[:, 1:][tie])            # equal scores in ascending row order
    r1, d1 = ev.top1(*b)
    assert np.array_equal(r[:, 0], r1) and np.array_equal(d[:, 0].view(np.uint32), d1.view(np.uint32))
    ev.close()


def test_nearest_text_and_cli(gpu, tmp_path):
    """Evaluator.nearest_text and ./nearest (binary and bit-packed input) print the same bytes, and those are the
    oracle's rows and scores in the documented format."""
    E = eval_oracle()
    words, M = read_vectors(os.path.join(GOLDEN, "b1_d8.vec"), 1)
    c = w2b.Corpus(os.path.join(GOLDEN, "corpus_small.txt"), 2)
    assert c.words() == words
    binp, pk = str(tmp_path / "m.bin"), str(tmp_path / "m.w2bp")
    c.save_vectors(binp, M, 1)
    c.save_vectors_packed(pk, w2b.pack_quantized(M, 1), M.shape[1], 1)
    c.close()
    k = 6
    om, ev = E.EvalModel(binp, 0, 0, fma=True), w2b.Evaluator(binp, 0, 0)
    names = [n for n in om.names if n and om.lookup(n) < om.words][1:9]
    low = bytes.lower
    lines = [low(names[0]), b"  " + low(names[1]) + b"\t" + names[2] + b"   " + low(names[3]) + b" ", b"",
             names[4] + b" " + names[5], low(names[6]) + b" no-such-word also-missing", b"no-such-word",
             names[7] + b" " + names[7] + b" " + names[7]]
    queries = b"\n".join(lines) + b"\n"
    want = b""
    for ln in lines:
        tok = [t.upper() for t in ln.split()]
        if not tok:
            continue
        head = b" ".join(tok)
        if len(tok) not in (1, 3):
            want += head + b": expected 1 or 3 words\n"
            continue
        r = [om.lookup(t) for t in tok]
        if om.words in r:
            want += head + b": not in vocabulary: " + tok[r.index(om.words)] + b"\n"
            continue
        r = r * 3 if len(r) == 1 else r
        rows, scores = oracle_topk(om, [r[0]], [r[1]], [r[2]], k)
        want += head + b":\n"
        for j in range(k):
            if rows[0, j] < 0:
                break
            want += b"%d\t%s\t%s\n" % (j + 1, om.names[rows[0, j]], ("%.6f" % float(scores[0, j])).encode())
    got = ev.nearest_text(queries, k)
    ev.close()
    assert got == want
    assert got.count(b":\n") == 3
    for f in (binp, pk):
        r = subprocess.run([CLI, f, str(k)], input=queries, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, f
    r = subprocess.run([CLI, str(tmp_path / "missing.bin"), "3"], input=b"", capture_output=True, timeout=300)
    assert r.stdout == b"Input file not found\n" and r.returncode == 255
