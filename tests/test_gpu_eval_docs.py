"""The document question on the GPU (include/word2bits_eval.h, w2b_eval_docs): both packed modes against the host twin's score
of every document, sorted here; the two identities of the header (one-id texts = the bag question, permutations change no
bit); the rounding regime of the bits score; the scratch bound, replacing and dropping the corpus, the text form and the
command line, the refusals and the timing.  Documents are compared exactly and score bits bit for bit; no tolerance anywhere.

Shapes.  Row lengths: 1; 64 and 65 (a last block of one column); 200 (the query row of a table column in registers on both
handle kinds); 513 (in memory on both: more than 16 halves).  The walk cuts a wavefront into groups of 16, 32 or 64 lanes by
the query's ids >= 0: queries of 1, 2 and 16 ids take groups of 16, of 17, 20 and 32 ids groups of 32 (the benchmark's path),
of 33, 48, 49, 62 and 63 ids one group of 64; 65 and about 920 ids walk a document once per 64-column tile; one query is all
padding.  Documents have 0 .. 1024 positions.  3001 documents are three walk workgroups, the last one partial, whose
lists meet in the merge; 257 documents are one partial workgroup.

The rounding regime: the issue's shape D = 16448 cannot produce an odd R (D even makes every I even), so beside it stands D =
16449 with a query of 1023 ids: R is then a sum of 1023 odd numbers, odd, and above 2^24 for near-identical rows."""
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
from docs_testlib import MAX_DOC, answer_list, flatten, host_docs, make_docs, make_model

pytestmark = pytest.mark.gpu
NEAR = os.path.join(ROOT, "nearest")
SHORT = [0, 1, 2, 2, 1, 63, 64, 65]
# (bitlevel, D, V, n_docs)
CASES = [(1, 200, 300, 257), (2, 200, 300, 257), (1, 513, 300, 257), (2, 513, 5, 2), (1, 64, 300, 3001), (2, 64, 5, 257),
         (1, 1, 5, 1), (2, 1, 300, 2), (1, 65, 5, 2), (2, 65, 300, 1)]
# query lengths: both sides of 16 | 17 and of 32 | 33 ids (the walk's groups of 16, 32 and 64 lanes; 20 is the benchmark's
# length), of 48 | 49 (a 64-lane group partly filled), of 64 | 65 (one tile, two tiles), and the longest text
QLENS = (1, 2, 63, 64, 65, MAX_DOC, 16, 17, 20, 32, 33, 48, 49)
_cache = {}


def names_of(n):
    return [b"w%d" % i for i in range(n)]


def handle(tmp_path, bitlevel, packed, D):
    lib = bits_testlib if bitlevel == 1 else codes_testlib
    path = lib.write_packed_file(str(tmp_path / ("m%d.w2bp" % bitlevel)), names_of(packed.shape[0]), packed, D)
    return w2b.Evaluator(path, bits=bitlevel == 1, codes=bitlevel == 2), path


def twin_scores(packed, D, bitlevel, ids, offsets, queries):
    """float32 [2 (symmetric)][nq][n_docs] from the host twin"""
    out = []
    for symmetric in (0, 1):
        rows = []
        for q in queries:
            rc, _, sc = host_docs(packed, D, bitlevel, ids, offsets, q, symmetric, want_dir=False)
            assert rc == 0
            rows.append(sc)
        out.append(np.stack(rows))
    return out


def batch(bitlevel, D, V, n_docs):
    """the model, its corpus, its queries and the twin's score of every (query, document) -- computed once, never changed"""
    key = (bitlevel, D, V, n_docs)
    if key not in _cache:
        rng = np.random.default_rng(hash(key) % 2 ** 32)
        M, packed = make_model(rng, bitlevel, V, D)
        lengths = ([MAX_DOC, 65, 64, 63, 2, 1, 0, MAX_DOC] + SHORT * (n_docs // len(SHORT) + 1))[:n_docs]
        if n_docs <= 2:
            lengths = [MAX_DOC, 3][:n_docs]
        docs = make_docs(rng, V, n_docs, lengths) if n_docs > 2 else [rng.integers(0, V, n).astype(np.int32) for n in lengths]
        queries = [rng.integers(0, V, n).astype(np.int32) for n in QLENS]
        queries[3][[1, 9]] = -1                                   # padding inside a query
        queries[5][rng.random(MAX_DOC) < 0.1] = -1
        queries.append(np.full(6, -1, np.int32))                  # all padding
        if n_docs >= 200:                                         # three copies of query 2: the best score, three times
            docs[7], docs[100], docs[101] = queries[2].copy(), queries[2].copy(), queries[2][::-1].copy()
        ids, offsets = flatten(docs)
        S = twin_scores(packed, D, bitlevel, ids, offsets, queries)
        for a in (packed, ids, offsets, *queries, *S):
            a.setflags(write=False)
        _cache[key] = (M, packed, docs, ids, offsets, queries, S)
    return _cache[key]


def expected(S, k):
    rows, out = np.empty((len(S), k), np.int32), np.empty((len(S), k), np.float32)
    for q in range(len(S)):
        rows[q], out[q] = answer_list(S[q], k)
    return rows, out


def check(got, want):
    (gr, gd), (wr, wd) = got[:2], want[:2]
    assert gr.shape == wr.shape and gd.shape == wd.shape
    assert np.array_equal(gr, wr), np.argwhere(gr != wr)[:10]
    assert same_floats(gd, wd)


@pytest.mark.parametrize("bitlevel,D,V,n_docs", CASES)
def test_lists_and_all_scores_equal_the_host_twin(gpu, bitlevel, D, V, n_docs, tmp_path):
    M, packed, docs, ids, offsets, queries, S = batch(bitlevel, D, V, n_docs)
    qids, qoff = flatten(queries)
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    ev.set_docs(ids, offsets)
    assert ev.docs_count() == n_docs
    short_tail = False
    for symmetric in (0, 1):
        for k in (1, 10, 64):
            got = ev.docs(qids, qoff, k, symmetric=bool(symmetric), all_scores=True)
            assert np.array_equal(got[2].view(np.uint32), S[symmetric].view(np.uint32)), (symmetric, k)
            want = expected(S[symmetric], k)
            check(got, want)
            check(ev.docs(qids, qoff, k, symmetric=bool(symmetric)), want)
            assert np.all(got[0][-1] == -1) and not got[1][-1].view(np.uint32).any()       # the all-padding query
            short_tail |= bool(np.any((want[0][:-1, 0] >= 0) & (want[0][:-1, -1] < 0)))
    assert short_tail or n_docs > 64                              # k above the number of answers: a tail of -1 / 0
    if n_docs >= 200:                                             # duplicate documents: equal scores, ascending index
        r = ev.docs(qids, qoff, 64)[0]
        assert np.array_equal(S[1][:, 7].view(np.uint32), S[1][:, 100].view(np.uint32))
        assert np.array_equal(S[1][:, 7].view(np.uint32), S[1][:, 101].view(np.uint32))
        for q in range(len(queries) - 1):
            at = [int(np.flatnonzero(r[q] == d)[0]) for d in (7, 100, 101) if d in r[q]]
            assert at == sorted(at)
        assert V == 5 or list(r[2][:3]) == [7, 100, 101]          # (five words: other documents cover the query as well)
    ev.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("D", [65, 200])
def test_one_id_texts_equal_the_bag_question(gpu, bitlevel, D, tmp_path):
    V = 300
    M, packed = make_model(np.random.default_rng(D + bitlevel), bitlevel, V, D)
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    ev.set_docs(np.arange(V), np.arange(V + 1))
    rows = np.random.default_rng(D).integers(0, V, 40).astype(np.int32)
    for k in (1, 10, 64):
        want = ev.bag(rows, np.arange(41), k, exclude_own=False)
        for symmetric in (False, True):
            check(ev.docs(rows, np.arange(41), k, symmetric=symmetric), want)
    ev.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_permutations_change_no_bit(gpu, bitlevel, tmp_path):
    M, packed, docs, ids, offsets, queries, S = batch(bitlevel, 200, 300, 257)
    rng = np.random.default_rng(5)
    qids, qoff = flatten(queries)
    ev, _ = handle(tmp_path, bitlevel, packed, 200)
    ev.set_docs(ids, offsets)
    want = ev.docs(qids, qoff, 10, all_scores=True)
    ev.set_docs(flatten([rng.permutation(d) for d in docs])[0], offsets)
    got = ev.docs(flatten([rng.permutation(q) for q in queries])[0], qoff, 10, all_scores=True)
    check(got, want)
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    ev.close()


@pytest.mark.parametrize("D,mq", [(16448, 1024), (16449, 1023)])
def test_bits_rounding_regime(gpu, D, mq, tmp_path):
    V = 8
    rng = np.random.default_rng(D)
    M = np.tile((rng.integers(0, 2, (1, D)) * 2 - 1).astype(np.int8), (V, 1))
    for r in range(1, V):
        M[r, rng.integers(0, D, r)] *= -1                        # near-identical rows
    packed = bits_testlib.pack_signs(M)
    q = np.concatenate([rng.integers(0, V, mq), np.full(MAX_DOC - mq, -1)]).astype(np.int32)
    docs = [np.full(MAX_DOC, 3, np.int32), np.array([1, 2, 5], np.int32), rng.integers(0, V, 100).astype(np.int32)]
    ids, offsets = flatten(docs)
    S = []
    for symmetric in (0, 1):
        rc, R, sc = host_docs(packed, D, 1, ids, offsets, q, symmetric)
        assert rc == 0
        S.append(sc)
    assert R.max() > 2 ** 24
    if D % 2:
        big = R[R > 2 ** 24]
        assert np.any(big % 2 == 1)                              # not a float32: (float)R rounds
        assert np.any(np.float32(big).astype(np.int64) != big)
    ev, _ = handle(tmp_path, 1, packed, D)
    ev.set_docs(ids, offsets)
    for symmetric in (0, 1):
        got = ev.docs(q, [0, MAX_DOC], 3, symmetric=bool(symmetric), all_scores=True)
        assert np.array_equal(got[2][0].view(np.uint32), S[symmetric].view(np.uint32))
        check(got, expected(S[symmetric][None, :], 3))
    ev.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_scratch_bound_corpus_replacement_timing_and_refusals(gpu, bitlevel, tmp_path):
    D, V, k = 200, 300, 10
    M, packed, docs, ids, offsets, queries, S = batch(bitlevel, D, V, 257)
    qids, qoff = flatten(queries)
    nq = len(queries)
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    probe = np.arange(20, dtype=np.int32)
    before = ev.topk(probe, probe[::-1].copy(), probe, 5)
    ev.set_docs(ids, offsets)
    ev.timing()
    want = ev.docs(qids, qoff, k, all_scores=True)
    check(want, expected(S[1], k))
    ms, launches, macs = ev.timing()
    assert launches == 1 and ms > 0 and macs == float(len(qids)) * float(len(ids)) * D
    table_ms, walk_ms = ev.docs_timing()
    assert table_ms > 0 and walk_ms > 0 and table_ms + walk_ms == ms
    ev.set_topk_scratch(1)                                        # the smallest bound: one query per chunk
    got = ev.docs(qids, qoff, k, all_scores=True)
    check(got, want)
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert ev.timing()[1] == nq
    ev.set_topk_scratch(0)
    check(ev.docs(qids, qoff, k), want)
    check(ev.topk(probe, probe[::-1].copy(), probe, 5), before)   # the other questions of the handle are untouched

    # another corpus replaces the first; an empty one drops it
    sub_ids, sub_off = flatten(docs[200:230])
    ev.set_docs(sub_ids, sub_off)
    assert ev.docs_count() == 30
    check(ev.docs(qids, qoff, k), expected(S[1][:, 200:230], k))
    L = _lib.lib()
    best, bestd = np.full((nq, k), -5, np.int32), np.full((nq, k), -5, np.float32)
    every = np.full((nq, 30), -5, np.float32)
    bp, dp, ep = best.ctypes.data_as(_lib.i32p), bestd.ctypes.data_as(_lib.f32p), every.ctypes.data_as(_lib.f32p)
    bad = qids.copy()
    bad[-1] = V
    assert L.w2b_eval_docs(ev._h, len(bad), bad.ctypes.data_as(_lib.i32p), nq, qoff.ctypes.data_as(_lib.i64p), 1, k, bp, dp,
                           ep) == _lib.W2B_EINVAL and b"query id out of range" in L.w2b_last_error()
    assert np.all(best == -5) and np.all(bestd == -5) and np.all(every == -5)
    for call, msg in ((lambda: ev.docs(qids, qoff, 0), "k must be 1..64"), (lambda: ev.docs(qids, qoff, 65), "k must be 1..64"),
                      (lambda: ev.docs(qids, qoff, k, symmetric=2), "symmetric must be 0 or 1"),
                      (lambda: ev.docs(np.zeros(MAX_DOC + 1, np.int32), [0, MAX_DOC + 1], k), "a query holds at most 1024"),
                      (lambda: ev.docs([0, 1], [0, 1], k), "offsets must start at 0"),
                      (lambda: ev.set_docs(np.zeros(MAX_DOC + 1, np.int32), [0, MAX_DOC + 1]), "a document holds at most 1024"),
                      (lambda: ev.set_docs([0, V], [0, 2]), "document id out of range")):
        with pytest.raises(w2b.W2bError) as e:
            call()
        assert e.value.code == _lib.W2B_EINVAL and msg in str(e.value)
    assert ev.docs_count() == 30                                  # a refused corpus leaves the earlier one
    r, d = ev.docs([], [0], k)                                    # no queries
    assert r.shape == (0, k) and d.shape == (0, k)
    ev.set_docs([], [0])
    assert ev.docs_count() == 0
    r, d = ev.docs([], [0], k)                                    # no queries: nothing is asked, no corpus is needed
    assert r.shape == (0, k)
    with pytest.raises(w2b.W2bError) as e:
        ev.docs(qids, qoff, k)
    assert e.value.code == _lib.W2B_EINVAL and "no corpus is set" in str(e.value)
    ev.close()


def test_limits_that_depend_on_the_handle(gpu, tmp_path):
    """all_scores holds at most 2^28 scores; a handle of size >= 2^21 is refused"""
    L = _lib.lib()
    M, packed = make_model(np.random.default_rng(1), 1, 8, 65)
    ev, _ = handle(tmp_path, 1, packed, 65)
    n_docs, nq, k = (1 << 20) + 1, 256, 2
    ev.set_docs([], np.zeros(n_docs + 1, np.int64))               # documents without positions
    qoff = np.zeros(nq + 1, np.int64)
    best, bestd, every = np.full((nq, k), -5, np.int32), np.full((nq, k), -5, np.float32), np.full(4, -5, np.float32)
    none = np.zeros(1, np.int32)
    assert nq * n_docs > 1 << 28
    rc = L.w2b_eval_docs(ev._h, 0, none.ctypes.data_as(_lib.i32p), nq, qoff.ctypes.data_as(_lib.i64p), 1, k,
                         best.ctypes.data_as(_lib.i32p), bestd.ctypes.data_as(_lib.f32p), every.ctypes.data_as(_lib.f32p))
    assert rc == _lib.W2B_EINVAL and b"all_scores holds at most 2^28 scores" in L.w2b_last_error()
    assert np.all(best == -5) and np.all(bestd == -5) and np.all(every == -5)
    r, d = ev.docs([], qoff[:256], k, all_scores=False)           # one query fewer: (2^20 + 1) * 255 < 2^28, and without
    assert np.all(r == -1) and not d.view(np.uint32).any()        # all_scores there is no such limit anyway
    ev.close()
    D = 1 << 21
    big = np.zeros((2, D // 64), np.uint64)
    path = bits_testlib.write_packed_file(str(tmp_path / "big.w2bp"), names_of(2), big, D)
    ev = w2b.Evaluator(path, bits=True)
    for call in (lambda: ev.set_docs([0, 1], [0, 2]), lambda: ev.docs([0], [0, 1], 1)):
        with pytest.raises(w2b.W2bError) as e:
            call()
        assert e.value.code == _lib.W2B_EINVAL and "size must be below 2^21" in str(e.value)
    ev.close()


def test_fp32_handle_refuses(gpu, tmp_path):
    rng = np.random.default_rng(8)
    path = write_vectors_file(str(tmp_path / "m.bin"), names_of(40), seeded_matrix(rng, "1bit", 40, 20))
    ev = w2b.Evaluator(path, 0, 0)
    for call in (lambda: ev.set_docs([1, 2], [0, 2]), lambda: ev.docs([1, 2], [0, 2], 3), lambda: ev.set_docs_text(b"w1 w2\n"),
                 lambda: ev.docs_text(b"w1 w2\n", 3)):
        with pytest.raises(w2b.W2bError) as e:
            call()
        assert e.value.code == _lib.W2B_EINVAL
        assert "not available on an fp32 handle: load the file with bits or codes" in str(e.value)
    ev.close()


def listing(head, score, k):
    r, d = answer_list(score, k)
    return head + b":\n" + b"".join(b"%d\t%d\t%s\n" % (j + 1, r[j] + 1, ("%.6f" % float(d[j])).encode())
                                    for j in range(k) if r[j] >= 0)


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_text_form_and_command_line(gpu, bitlevel, tmp_path):
    D, V, k = 65, 300, 5
    rng = np.random.default_rng(40 + bitlevel)
    M, packed = make_model(rng, bitlevel, V, D)
    ev, path = handle(tmp_path, bitlevel, packed, D)
    docs = [rng.integers(0, V, n).astype(np.int32) for n in (5, 0, 12, 1, 30, 7, 7, 3, 9, 2, 40, 6)]
    lines = [b" ".join(b"w%d" % i for i in d) for d in docs]
    lines[2] += b" nosuch  Other"                                 # dropped words; the empty line 2 is document 1
    lines[4] = lines[4].replace(b"w", b"W", 3)
    corpus = b"\n".join(lines) + b"\n"
    assert ev.set_docs_text(corpus) == (len(docs), 2) and ev.docs_count() == len(docs)
    ids, offsets = flatten(docs)
    qs = [np.array([3], np.int32), docs[4][:10], np.array([8, 9], np.int32)]
    queries = b"w3\n" + b" ".join(b"w%d" % i for i in qs[1]) + b" unknown\nnosuch either\n\nW8  w9"
    heads = [b"W3", b" ".join(b"W%d" % i for i in qs[1]) + b" UNKNOWN", b"W8 W9"]
    for symmetric in (1, 0):
        sc = [host_docs(packed, D, bitlevel, ids, offsets, q, symmetric)[2] for q in qs]
        want = (listing(heads[0], sc[0], k) + listing(heads[1], sc[1], k) + b"NOSUCH EITHER: no word in vocabulary\n" +
                listing(heads[2], sc[2], k))
        assert want.count(b"\n") > 2 * k
        assert ev.docs_text(queries, k, symmetric=bool(symmetric)) == want
        cpath = str(tmp_path / "corpus.txt")
        open(cpath, "wb").write(corpus)
        r = subprocess.run([NEAR, path, str(k), "0", "0", "bits" if bitlevel == 1 else "codes", "docs", cpath] +
                           ([] if symmetric else ["oneway"]), input=queries, capture_output=True, timeout=300)
        assert r.returncode == 0 and r.stdout == want, r.stderr
        assert b"2 words outside the vocabulary dropped" in r.stderr
    long_line = b" ".join([b"w1"] * (MAX_DOC + 1))
    assert ev.docs_text(long_line + b"\n", k) == long_line.upper() + b": expected at most 1024 words\n"
    with pytest.raises(w2b.W2bError) as e:                        # an over-long line: refused, naming it; the corpus stays
        ev.set_docs_text(b"w1 w2\n\n" + long_line + b"\n")
    assert e.value.code == _lib.W2B_EINVAL and "line 3" in str(e.value)
    assert ev.docs_count() == len(docs)
    assert ev.docs_text(b"w3\n", k) == listing(b"W3", host_docs(packed, D, bitlevel, ids, offsets, qs[0], 1)[2], k)
    r = subprocess.run([NEAR, path, str(k), "0", "0", "bits" if bitlevel == 1 else "codes", "docs", str(tmp_path / "missing.txt")],
                       input=queries, capture_output=True, timeout=300)
    missing_model = subprocess.run([NEAR, str(tmp_path / "nomodel.bin"), str(k)], input=b"", capture_output=True, timeout=300)
    assert r.stdout == b"Corpus file not found\n" and r.returncode == missing_model.returncode != 0
    ev.close()
