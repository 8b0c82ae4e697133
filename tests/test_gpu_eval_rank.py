"""Rank of a given row on the GPU (include/word2bits_eval.h, "rank of a given row"): ranks and tie counts as integers and
score bits exactly equal to the host twin's (tests/test_eval_rank_host.py ties the twin to the numpy definition, and so does
every case here once more); no tolerance anywhere.  V = 300 is five row splits of the 1-bit scan and two workgroups of the
2-bit scan with a partial last tile; Q = 40 is a partial second question tile."""
import os
import re
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT, write_vectors_file
import bits_testlib
import codes_testlib
from rank_testlib import (CASES, NAMES, Q, V, all_scores, case, full_list, host_rank, host_truth, same_bits, truth_from_scores,
                          write_model)

pytestmark = pytest.mark.gpu
ACC, NEAR = (os.path.join(ROOT, n) for n in ("compute_accuracy", "nearest"))
SMALLEST = {1: 1, 2: 1}


@pytest.fixture
def handle(gpu, tmp_path):
    made = []

    def open_(bitlevel, D):
        packed = case(bitlevel, D)[1]
        path = write_model(str(tmp_path / ("m%d_%d.w2bp" % (bitlevel, D))), bitlevel, packed, D)
        ev = w2b.Evaluator(path, bits=bitlevel == 1, codes=bitlevel == 2)
        assert (ev.words, ev.size) == (V, D)
        made.append(ev)
        return ev

    yield open_
    for ev in made:
        ev.close()


def check(got, want):
    (gr, gt, gs), (wr, wt, ws) = got, want
    assert gr.dtype == np.int32 and gt.dtype == np.int32 and gs.dtype == np.float32
    assert np.array_equal(gr, wr), (np.flatnonzero(gr != wr)[:10], gr[gr != wr][:10], wr[gr != wr][:10])
    assert np.array_equal(gt, wt), (np.flatnonzero(gt != wt)[:10], gt[gt != wt][:10], wt[gt != wt][:10])
    assert same_bits(gs, ws)


@pytest.mark.parametrize("bitlevel,D", CASES)
def test_ranks_equal_the_host_twin(handle, bitlevel, D):
    _, packed, b, g, _, truth = case(bitlevel, D)
    want = host_truth(packed, D, bitlevel, b, g)
    check(want, truth)                                          # the twin is the numpy definition
    ev = handle(bitlevel, D)
    check(ev.rank(*b, g, details=True), want)
    assert np.array_equal(ev.rank(*b, g), want[0])              # without details: the ranks alone (NULL tied / score)


@pytest.mark.parametrize("bitlevel,D", CASES)
def test_overlap_with_topk_in_both_directions(handle, bitlevel, D):
    _, _, b, g, _, _ = case(bitlevel, D)
    ev = handle(bitlevel, D)
    rank, _, score = ev.rank(*b, g, details=True)
    rows, sc = ev.topk(*b, 64)
    inside = 0
    for q in range(Q):
        at = np.flatnonzero(rows[q] == g[q])
        if 1 <= rank[q] <= 64:                                  # a rank within the list: that place holds the target
            assert list(at) == [rank[q] - 1], q
            assert same_bits(sc[q, rank[q] - 1], score[q]), q
            inside += 1
        else:                                                   # no rank, or one beyond the list: the target is not in it
            assert len(at) == 0, q
    assert inside >= 3 and (rank > 64).sum() >= 3 and (rank == 0).sum() >= 3


@pytest.mark.parametrize("bitlevel,D", [(1, 200), (1, SMALLEST[1]), (2, 200), (2, SMALLEST[2])])
def test_every_row_as_target_of_one_question(handle, bitlevel, D):
    M, _, b, _, S, _ = case(bitlevel, D)
    ev = handle(bitlevel, D)
    block = np.arange(V // 3, V // 3 + max(2, V // 10))
    all_rows = np.arange(V, dtype=np.int32)
    # a question whose complete list reaches the block of identical rows, and one with b1 == b2 == b3
    reach = [q for q in range(Q) if len(np.intersect1d(full_list(S, q, *b), block)) >= 2]
    assert reach
    for q in (reach[0], 2):
        bq = np.repeat(b[:, q:q + 1], V, axis=1)
        rank, tied, score = ev.rank(*bq, all_rows, details=True)
        want = truth_from_scores(np.repeat(S[q:q + 1], V, axis=0), bitlevel, D, *bq, all_rows)
        check((rank, tied, score), want)
        order = full_list(S, q, *b)
        m = len(order)
        assert sorted(rank[rank > 0]) == list(range(1, m + 1)) and (rank == 0).sum() == V - m
        assert np.array_equal(all_rows[rank > 0][np.argsort(rank[rank > 0])], order)
        in_list = np.array([r for r in block if rank[r] > 0])
        if len(in_list) >= 2:                                   # identical rows: consecutive places in row order, tied alike
            assert np.array_equal(np.diff(rank[in_list]), np.ones(len(in_list) - 1, np.int32))
            assert np.all(tied[in_list] == tied[in_list[0]]) and tied[in_list[0]] >= len(in_list) - 1
            assert len(set(score[in_list].view(np.uint32).tolist())) == 1
        own = set(int(x) for x in b[:, q])
        assert all(rank[r] == 0 for r in own)


@pytest.mark.parametrize("bitlevel,D", CASES)
def test_tiled_questions_and_the_scratch_bound(handle, bitlevel, D):
    _, _, b, g, _, truth = case(bitlevel, D)
    ev = handle(bitlevel, D)
    bt, gt = np.tile(b, (1, 15)), np.tile(g, 15)                # 600 questions: several question blocks / tile ranges
    want = tuple(np.tile(x, 15) for x in truth)
    ev.timing()
    check(ev.rank(*bt, gt, details=True), want)
    ms, launches, macs = ev.timing()
    assert launches == 1 and ms > 0 and macs == (3.0 if bitlevel == 2 else 1.0) * 600 * V * D
    ev.set_topk_scratch(1)                                      # a bound that forces 128-question chunks
    check(ev.rank(*bt, gt, details=True), want)
    assert ev.timing()[1] == (600 + 127) // 128
    ev.set_topk_scratch(0)
    check(ev.rank(*bt, gt, details=True), want)
    assert ev.timing()[1] == 1


@pytest.mark.parametrize("bitlevel,D", [(1, 200), (1, 1030), (2, 200), (2, 417)])
def test_neighbor_rank_is_rank_with_one_row_three_times(handle, bitlevel, D):
    _, packed, b, g, _, _ = case(bitlevel, D)
    ev = handle(bitlevel, D)
    rows = b[0]
    got = ev.neighbor_rank(rows, g, details=True)
    check(got, ev.rank(rows, rows, rows, g, details=True))
    check(got, host_truth(packed, D, bitlevel, np.stack([rows, rows, rows]), g))
    assert np.array_equal(ev.neighbor_rank(rows, g), got[0])
    assert np.all(ev.neighbor_rank(rows, rows) == 0)            # a row is not its own neighbour


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_refusals_leave_the_outputs_untouched(handle, bitlevel, tmp_path):
    D = 65
    M, _, b, g, _, truth = case(bitlevel, D)
    ev = handle(bitlevel, D)
    L = _lib.lib()
    rank, tied, score = np.full(Q, 77, np.int32), np.full(Q, 77, np.int32), np.full(Q, 7.5, np.float32)
    ip = lambda a: a.ctypes.data_as(_lib.i32p)

    def call(h, rows, tgt, n=Q, out=(rank, tied, score)):
        keep = [np.ascontiguousarray(x, np.int32) for x in (*rows, tgt)]
        rc = L.w2b_eval_rank(h, n, *(ip(x) for x in keep), ip(out[0]), None if out[1] is None else ip(out[1]),
                             None if out[2] is None else out[2].ctypes.data_as(_lib.f32p))
        return rc, L.w2b_last_error()

    rc, why = call(ev._h, b, g, n=-1)
    assert rc == _lib.W2B_EINVAL and b"bad argument" in why
    rc, why = call(None, b, g, n=-1)                            # a NULL handle with a bad count: the count is reported
    assert rc == _lib.W2B_EINVAL and b"bad argument" in why
    rc, why = call(None, b, g)
    assert rc == _lib.W2B_EINVAL and b"null handle" in why
    for slot in range(4):
        for bad_row in (V, -1):
            bb, gg = b.copy(), g.copy()
            (bb[slot] if slot < 3 else gg)[17] = bad_row
            rc, why = call(ev._h, bb, gg)
            assert rc == _lib.W2B_EINVAL and b"question 17" in why and b"row out of range" in why, (slot, bad_row)
    lib = bits_testlib if bitlevel == 1 else codes_testlib
    fl = write_vectors_file(str(tmp_path / "m.bin"), NAMES, lib.values_of(M))
    f32 = w2b.Evaluator(fl, bitlevel, 0)
    try:
        rc, why = call(f32._h, b, g)
        assert rc == _lib.W2B_EINVAL and b"not available on an fp32 handle: load the file with bits or codes" in why
        for f in (lambda: f32.rank_text(b"w1 w2\n"), lambda: f32.transcript(b": s\nw1 w2 w3 w4\n", method="rank"),
                  lambda: f32.neighbor_rank([1], [2])):
            with pytest.raises(w2b.W2bError) as e:
                f()
            assert e.value.code == _lib.W2B_EINVAL and "fp32 handle" in str(e.value)
    finally:
        f32.close()
    assert np.all(rank == 77) and np.all(tied == 77) and np.all(score == 7.5)
    # NULL tied / score are accepted, one at a time too
    rc, _ = call(ev._h, b, g, out=(rank, None, None))
    assert rc == _lib.W2B_OK and np.array_equal(rank, truth[0]) and np.all(tied == 77) and np.all(score == 7.5)
    rc, _ = call(ev._h, b, g, out=(rank, tied, None))
    assert rc == _lib.W2B_OK and np.array_equal(tied, truth[1]) and np.all(score == 7.5)
    rc, _ = call(ev._h, b, g, out=(rank, None, score))
    assert rc == _lib.W2B_OK and same_bits(score, truth[2])
    assert ev.rank(*b[:, :0], g[:0]).shape == (0,)              # no question: W2B_OK
    with pytest.raises(ValueError):
        ev.rank(b[0], b[1], b[2], g[:5])


def ranks_lines(sections, rank_of):
    """the RANKS lines of a transcript whose sections hold the given question indices, recomputed from the ranks: sums of
    1 / rank in stream order, in double"""
    def mean(total, n):
        return b"nan" if n == 0 else ("%.4f" % (total / float(n))).encode()

    out = []
    tot = [0.0, 0, 0.0, 0, 0.0, 0]                              # all, semantic, syntactic: sum and count
    for qid, qs in enumerate(sections, 1):
        s, h1, h5, h10, unr = 0.0, 0, 0, 0, 0
        for q in qs:
            r = int(rank_of[q])
            rr = 1.0 / r if r > 0 else 0.0
            s += rr
            tot[0] += rr
            tot[1] += 1
            k = 2 if qid <= 5 else 4
            tot[k] += rr
            tot[k + 1] += 1
            h1, h5, h10, unr = h1 + (r == 1), h5 + (1 <= r <= 5), h10 + (1 <= r <= 10), unr + (r == 0)
        out.append(b"RANKS section: MRR %s   hits@1 %d   hits@5 %d   hits@10 %d   unranked %d   (%d questions)\n" %
                   (mean(s, len(qs)), h1, h5, h10, unr, len(qs)))
        out.append(b"RANKS total: MRR %s   Semantic MRR %s   Syntactic MRR %s\n" %
                   (mean(tot[0], tot[1]), mean(tot[2], tot[3]), mean(tot[4], tot[5])))
    return out


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_text_forms_and_command_lines(handle, bitlevel, tmp_path):
    D = 200
    _, packed, b, g, _, truth = case(bitlevel, D)
    mode = "bits" if bitlevel == 1 else "codes"
    ev = handle(bitlevel, D)
    path = str(tmp_path / ("m%d_%d.w2bp" % (bitlevel, D)))
    ranked = [q for q in range(Q) if truth[0][q] > 0]
    qa, qb = ranked[0], ranked[-1]
    n_rc, n_rank, n_tied, n_score = host_rank(packed, D, bitlevel, b[0, qb], b[0, qb], b[0, qb], g[qb])
    assert n_rc == 0

    def answer(words, r, t, s):
        head = b" ".join(b"W%d" % w for w in words)
        return head + (b": no rank\n" if r == 0 else b":\t%d\t%d\t%s\n" % (r, t, ("%.6f" % float(s)).encode()))

    queries = (b"w%d w%d  w%d\tw%d\n" % (*b[:, qa], g[qa]) + b"w7\n\nw4 w5 w6\n" + b"W%d w%d\n" % (b[0, qb], g[qb]) +
               b"w1 no-such-word w2 nor-this\nw3 nope\n" + b"w%d w%d w%d w%d\n" % (*b[:, 0], g[0]) + b"w9 w9\n")
    want = (answer([*b[:, qa], g[qa]], truth[0][qa], truth[1][qa], truth[2][qa]) +
            b"W7: expected 2 or 4 words\nW4 W5 W6: expected 2 or 4 words\n" + answer([b[0, qb], g[qb]], n_rank, n_tied, n_score) +
            b"W1 NO-SUCH-WORD W2 NOR-THIS: not in vocabulary: NO-SUCH-WORD\nW3 NOPE: not in vocabulary: NOPE\n" +
            answer([*b[:, 0], g[0]], 0, 0, 0) + b"W9 W9: no rank\n")
    assert truth[0][0] == 0 and b"no rank" in want
    text = ev.rank_text(queries)
    assert text == want
    r = subprocess.run([NEAR, path, "10", "0", "0", mode, "rank"], input=queries, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == text, r.stderr

    # the transcript: six sections, the first and two more without a question, the last one syntactic (QID 6); one question
    # whose first word is not in the vocabulary is skipped
    line = lambda q: b"w%d w%d w%d w%d\n" % (*b[:, q], g[q])
    sections = [[], list(range(0, 14)), [], list(range(14, 20)), [], list(range(20, Q))]
    qs = b""
    for i, sec in enumerate(sections):
        qs += b": sec%d\n" % i + b"".join(line(q) for q in sec) + (b"nope w1 w2 w3\n" if i == 1 else b"")
    plain = ev.transcript(qs)
    got = ev.transcript(qs, method="rank")
    lines = got.splitlines(keepends=True)
    assert b"".join(l for l in lines if not l.startswith(b"RANKS")) == plain
    assert ev.transcript(qs) == plain                           # the default transcript is unchanged, before and after
    ranks = [l for l in lines if l.startswith(b"RANKS")]
    assert ranks == ranks_lines(sections, ev.rank(*b, g)) and np.array_equal(ev.rank(*b, g), truth[0])
    assert ranks[0].startswith(b"RANKS section: MRR nan ") and ranks[1] == b"RANKS total: MRR nan   Semantic MRR nan   Syntactic MRR nan\n"
    assert b"Syntactic MRR nan" in ranks[-3] and b"nan" not in ranks[-1]
    # every RANKS pair follows a "Total accuracy" line, and hits@1 is the count of the ACCURACY TOP1 line two lines above
    n_sections = 0
    for i, l in enumerate(lines):
        if l.startswith(b"RANKS section"):
            assert lines[i - 1].startswith(b"Total accuracy:") and lines[i + 1].startswith(b"RANKS total:")
            top1 = re.match(rb"ACCURACY TOP1: .* \((\d+) / (\d+)\)", lines[i - 2])
            assert top1 and int(re.search(rb"hits@1 (\d+) ", l).group(1)) == int(top1.group(1))
            n_sections += 1
    assert n_sections == len(sections)
    r = subprocess.run([ACC, path, "0", "0", mode, "rank"], input=qs, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == got, r.stderr
    with pytest.raises(ValueError):
        ev.transcript(qs, method="ranks")
