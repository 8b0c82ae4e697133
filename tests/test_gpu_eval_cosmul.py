"""3CosMul scoring on the GPU (include/word2bits_eval.h, "3CosMul"): rows and score bits exactly equal to the lists that the
host twin's scores sort into (tests/test_eval_cosmul_host.py ties the twin to the numpy definition, and so does every case
here once more); no tolerance anywhere.  V = 300 is five row splits of the 1-bit scan (the merge runs) and two workgroups of
the 2-bit scan with a partial last tile; Q = 40 is a partial second question tile."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT, eval_oracle, write_vectors_file
from topk_testlib import same_floats
import bits_testlib
import codes_testlib
from codes_testlib import truth_from_scores
from cosmul_testlib import TruthModel, host_scores, make_model, scores, write_model

pytestmark = pytest.mark.gpu
ACC, NEAR = (os.path.join(ROOT, n) for n in ("compute_accuracy", "nearest"))
V, Q = 300, 40
# 1-bit: 1024 | 1025 is the boundary between the three rows in registers and in memory
BITS_SIZES = [1, 2, 64, 65, 200, 1024, 1030]
# 2-bit: 416 | 417 is the boundary between two row tiles and one per wavefront, 1217 the first chunked size
CODES_SIZES = [1, 3, 32, 33, 64, 65, 200, 416, 417, 1217]
CASES = [(1, D) for D in BITS_SIZES] + [(2, D) for D in CODES_SIZES]
NAMES = [b"w%d" % i for i in range(V)]


@functools.lru_cache(maxsize=None)
def model(bitlevel, D):
    """(M, packed, b, S): the model, its questions and the host twin's scores [Q, V], computed once and left unchanged"""
    rng = np.random.default_rng(9000 + 10 * D + bitlevel)
    M, packed, b = make_model(rng, bitlevel, V, D, Q)
    S = np.stack([host_scores(packed, D, bitlevel, *b[:, q], want_u=False)[1] for q in range(Q)])
    assert np.array_equal(S.view(np.uint32), scores(M, bitlevel, *b).view(np.uint32))     # the numpy definition
    for a in (M, packed, b, S):
        a.setflags(write=False)
    return M, packed, b, S


@pytest.fixture
def handle(gpu, tmp_path):
    made = []

    def open_(bitlevel, D):
        _, packed, _, _ = model(bitlevel, D)
        path = write_model(str(tmp_path / ("m%d_%d.w2bp" % (bitlevel, D))), bitlevel, NAMES, packed, D)
        ev = w2b.Evaluator(path, bits=bitlevel == 1, codes=bitlevel == 2)
        assert (ev.words, ev.size) == (V, D)
        made.append(ev)
        return ev

    yield open_
    for ev in made:
        ev.close()


def check(got, want):
    (gr, gd), (wr, wd) = got, want
    assert gr.shape == wr.shape and gd.shape == wd.shape
    assert np.array_equal(gr, wr), np.argwhere(gr != wr)[:10]
    assert same_floats(gd, wd)


@pytest.mark.parametrize("bitlevel,D", CASES)
def test_lists_equal_the_sorted_host_twin_scores(handle, bitlevel, D):
    _, _, b, S = model(bitlevel, D)
    ev = handle(bitlevel, D)
    for k in (1, 10, 64):
        check(ev.cosmul(*b, k), truth_from_scores(S, *b, k))
    if bitlevel == 1:
        # the planted rows: the negation of question 0's b1 (u1 = 0: u2 * u3 / eps, far above every row with u1 >= 1 / D)
        # leads its list wherever it scores at all; the negation of question 1's b2 scores 0 and is no answer
        r, d = ev.cosmul(*b, 64)
        if D >= 64 and S[0, V - 1] > 0:
            assert r[0, 0] == V - 1 and d[0, 0] == S[0, V - 1] and d[0, 0] > 1.0
        assert S[1, V - 2] == 0 and V - 2 not in r[1]


@pytest.mark.parametrize("bitlevel,D", CASES)
def test_tiled_questions_scratch_bound_and_swapped_positives(handle, bitlevel, D):
    _, _, b, S = model(bitlevel, D)
    ev = handle(bitlevel, D)
    k = 10
    want = truth_from_scores(S, *b, k)
    # 600 questions: several question blocks (1-bit) / ranges of question tiles (2-bit) per launch; every copy has the list
    bt = np.tile(b, (1, 15))
    wt = tuple(np.tile(x, (15, 1)) for x in want)
    ev.timing()
    check(ev.cosmul(*bt, k), wt)
    assert ev.timing()[1] == 1
    # a scratch bound that forces 128-question chunks
    ev.set_topk_scratch(1)
    check(ev.cosmul(*bt, k), wt)
    assert ev.timing()[1] == (bt.shape[1] + 127) // 128
    ev.set_topk_scratch(0)
    # the two positives commute
    check(ev.cosmul(b[0], b[2], b[1], k), want)
    check(ev.cosmul(b[0], b[2], b[1], 64), truth_from_scores(S, *b, 64))


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_transcripts(handle, bitlevel, tmp_path):
    """transcript(method="cosmul") is the oracle's transcript() over a model whose top1 is the numpy 3CosMul truth; the
    default transcript stays the additive one, on the same handle, before and after."""
    E = eval_oracle()
    D = 200
    M, _, b, _ = model(bitlevel, D)
    lib = bits_testlib if bitlevel == 1 else codes_testlib
    fl = write_vectors_file(str(tmp_path / "m.bin"), NAMES, lib.values_of(M))
    om = E.EvalModel(fl, bitlevel, 0)
    rng = np.random.default_rng(31 + bitlevel)
    b4 = rng.integers(0, V, Q)
    qs = (b": capital\n" + b"".join(b"w%d w%d w%d w%d\n" % (*b[:, q], b4[q]) for q in range(Q // 2)) + b"nope w1 w2 w3\n: gram1\n" +
          b"".join(b"w%d w%d w%d w%d\n" % (*b[:, q], b4[q]) for q in range(Q // 2, Q)))
    ev = handle(bitlevel, D)
    add_truth = bits_testlib.TruthModel(om) if bitlevel == 1 else codes_testlib.TruthModel(om, M)
    want_add = E.transcript(add_truth, qs)
    assert ev.transcript(qs) == want_add
    want_mul = E.transcript(TruthModel(om, M, bitlevel), qs)
    got_mul = ev.transcript(qs, method="cosmul")
    assert got_mul == want_mul and b"ACCURACY TOP1" in got_mul
    assert ev.transcript(qs) == want_add and ev.transcript(qs, method="add") == want_add
    with pytest.raises(ValueError):
        ev.transcript(qs, method="mul")


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_text_form_and_command_lines(handle, bitlevel, tmp_path):
    D = 200
    _, packed, b, S = model(bitlevel, D)
    mode = "bits" if bitlevel == 1 else "codes"
    ev = handle(bitlevel, D)
    k = 10
    rows, sc = truth_from_scores(S, *b, k)
    queries = (b"w%d w%d  w%d\nw7\n\nw4 w5\nw1 no-such-word w2\n" % tuple(b[:, 0]) + b"W%d w%d w%d\n" % tuple(b[:, 5]))
    want = b""
    for q in (0,):
        want += b"W%d W%d W%d:\n" % tuple(b[:, q])
        want += b"".join(b"%d\tW%d\t%s\n" % (j + 1, rows[q, j], ("%.6f" % float(sc[q, j])).encode()) for j in range(k) if rows[q, j] >= 0)
    want += b"W7: expected 3 words\nW4 W5: expected 3 words\nW1 NO-SUCH-WORD W2: not in vocabulary: NO-SUCH-WORD\n"
    want += b"W%d W%d W%d:\n" % tuple(b[:, 5])
    want += b"".join(b"%d\tW%d\t%s\n" % (j + 1, rows[5, j], ("%.6f" % float(sc[5, j])).encode()) for j in range(k) if rows[5, j] >= 0)
    text = ev.cosmul_text(queries, k)
    assert text == want
    path = str(tmp_path / ("m%d_%d.w2bp" % (bitlevel, D)))
    r = subprocess.run([NEAR, path, str(k), "0", "0", mode, "cosmul"], input=queries, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == text, r.stderr
    qs = b": s\n" + b"".join(b"w%d w%d w%d w%d\n" % (*b[:, q], (q * 7) % V) for q in range(Q))
    r = subprocess.run([ACC, path, "0", "0", mode, "cosmul"], input=qs, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == ev.transcript(qs, method="cosmul"), r.stderr
    r = subprocess.run([ACC, path, "0", "0", mode], input=qs, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == ev.transcript(qs), r.stderr


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_refusals_leave_the_outputs_untouched(handle, bitlevel, tmp_path):
    D = 65
    M, _, b, _ = model(bitlevel, D)
    ev = handle(bitlevel, D)
    L = _lib.lib()
    best, bestd = np.full((Q, 64), 77, np.int32), np.full((Q, 64), 7.5, np.float32)
    p = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_lib.i32p)

    def call(h, rows, k):
        keep = [np.ascontiguousarray(x, np.int32) for x in rows]
        rc = L.w2b_eval_cosmul(h, Q, *(x.ctypes.data_as(_lib.i32p) for x in keep), k, best.ctypes.data_as(_lib.i32p),
                               bestd.ctypes.data_as(_lib.f32p))
        return rc, L.w2b_last_error()

    for bad_k in (0, 65):
        rc, why = call(ev._h, b, bad_k)
        assert rc == _lib.W2B_EINVAL and b"k must be 1..64" in why
        rc, why = call(None, b, bad_k)                          # a NULL handle with a bad k: the k is reported
        assert rc == _lib.W2B_EINVAL and b"k must be 1..64" in why
    rc, why = call(None, b, 5)
    assert rc == _lib.W2B_EINVAL and b"null handle" in why
    for bad_row in (V, -1):
        bb = b.copy()
        bb[1, 17] = bad_row
        rc, why = call(ev._h, bb, 5)
        assert rc == _lib.W2B_EINVAL and b"question 17" in why and b"row out of range" in why
    lib = bits_testlib if bitlevel == 1 else codes_testlib
    fl = write_vectors_file(str(tmp_path / "m.bin"), NAMES, lib.values_of(M))
    f32 = w2b.Evaluator(fl, bitlevel, 0)
    try:
        rc, why = call(f32._h, b, 5)
        assert rc == _lib.W2B_EINVAL and b"not available on an fp32 handle: load the file with bits or codes" in why
        for f in (lambda: f32.cosmul_text(b"w1 w2 w3\n", 5), lambda: f32.transcript(b": s\nw1 w2 w3 w4\n", method="cosmul")):
            with pytest.raises(w2b.W2bError) as e:
                f()
            assert e.value.code == _lib.W2B_EINVAL and "fp32 handle" in str(e.value)
    finally:
        f32.close()
    assert np.all(best == 77) and np.all(bestd == 7.5)
    with pytest.raises(w2b.W2bError):
        ev.cosmul(*b, 0)
    r, d = ev.cosmul(*b[:, :0], 5)                              # no question: W2B_OK
    assert r.shape == (0, 5) and d.shape == (0, 5)


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_timing_counts_the_launches(handle, bitlevel):
    D = 200
    _, _, b, _ = model(bitlevel, D)
    ev = handle(bitlevel, D)
    ev.timing()
    ev.cosmul(*b, 10)
    ms, launches, macs = ev.timing()
    assert launches == 1 and ms > 0 and macs == 3.0 * Q * V * D
    ev.cosmul(*b, 1)
    ev.cosmul(*b[:, :7], 64)
    ms, launches, macs = ev.timing()
    assert launches == 2 and ms > 0 and macs == 3.0 * (Q + 7) * V * D
    assert ev.timing() == (0.0, 0, 0.0)
