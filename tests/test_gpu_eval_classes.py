"""Word classes on the GPU (include/word2bits_eval.h, "word classes"): cls, the BIT PATTERNS of score, T_out, counts, iters_run
and moved all equal to the host twin (tests/test_eval_classes_host.py ties the twin to the numpy restatement); no tolerance
anywhere.  Shapes: sizes on both sides of the register-resident border (512 | 513), row counts that are no multiples of a
32-row tile (1000: four workgroups, 33: a second tile of one row), class counts around the borders of the 32-class tiles and
of their pairs."""
import functools
import os
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT, write_vectors_file
import bits_testlib
import codes_testlib
import classes_testlib as ct
from cosmul_testlib import write_model

pytestmark = pytest.mark.gpu
CLASSES = os.path.join(ROOT, "classes")
SIZES = [1, 65, 200, 512, 513, 800]
KS = [1, 2, 31, 32, 33, 65, 500]
GRID = [(b, D, V, K) for b in (1, 2) for D in SIZES for V in (1000, 33) for K in KS if K <= V]
GRID += [(b, D, 1, 1) for b in (1, 2) for D in (1, 65)]
ITERS = 4


@functools.lru_cache(maxsize=None)
def model(bitlevel, D, V):
    """(M, packed), computed once and left unchanged"""
    rng = np.random.default_rng(7300 + 10 * D + bitlevel + 100000 * V)
    if V >= 2:
        M, packed = ct.make_model(rng, bitlevel, V, D)
    else:
        M = (bits_testlib.make_signs if bitlevel == 1 else codes_testlib.make_codes)(rng, "random", V, D)
        packed = ct.pack(M, bitlevel)
    M.setflags(write=False)
    packed.setflags(write=False)
    return M, packed


@functools.lru_cache(maxsize=None)
def twin(bitlevel, D, V, K, iters):
    return ct.host_classes(model(bitlevel, D, V)[1], D, bitlevel, K, iters)


def names(V):
    return [b"w%d" % i for i in range(V)]


@pytest.fixture
def handle(gpu, tmp_path):
    made = []

    def open_(bitlevel, D, packed, threshold=0):
        V = packed.shape[0]
        path = write_model(str(tmp_path / ("m%d_%d_%d.w2bp" % (bitlevel, D, V))), bitlevel, names(V), packed, D)
        ev = w2b.Evaluator(path, threshold=threshold, bits=bitlevel == 1, codes=bitlevel == 2)
        assert ev.size == D and ev.words == (min(V, threshold) if threshold else V)
        made.append(ev)
        return ev

    yield open_
    for ev in made:
        ev.close()


def check(got, want):
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:10]
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), np.flatnonzero(got[1].view(np.uint32) != want[1].view(np.uint32))[:10]
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert (got[4], got[5]) == (want[4], want[5])


@pytest.mark.parametrize("bitlevel,D,V,K", GRID)
def test_every_output_equals_the_host_twin(handle, bitlevel, D, V, K):
    _, packed = model(bitlevel, D, V)
    ev = handle(bitlevel, D, packed)
    check(ev.classes(K, ITERS, details=True), twin(bitlevel, D, V, K, ITERS))
    assert np.array_equal(ev.classes(K, ITERS), twin(bitlevel, D, V, K, ITERS)[0])


@functools.lru_cache(maxsize=None)
def big(bitlevel, V, D):
    M, packed, _ = ct.planted(np.random.default_rng(77 + bitlevel), bitlevel, V, D, 2, 0.05)
    return M, packed, ct.host_classes(packed, D, bitlevel, 2, 3)


@pytest.mark.parametrize("bitlevel,V,D", [(2, 100000, 200), (1, 200000, 400)])
def test_the_rounding_regime_shows_the_chain_order(handle, bitlevel, V, D):
    """Two planted prototypes with 5 % flips, K = 2, max_iters = 3: from the second iteration on a class sum is about 0.9 V
    (0.9 V x up to 3 per column), so the partial sums pass 2^24 after a few dozen columns and every later step rounds: the
    order of the chain is visible in `score`.  First, on the CPU: the numpy restatement with the columns REVERSED changes at
    least one score bit pattern against the twin (which equals the restatement in column order: the host tests) -- so
    agreement of the GPU with the twin proves the order."""
    M, packed, want = big(bitlevel, V, D)
    assert np.abs(want[2]).max().astype(np.int64) * D > 2 ** 24
    rev = ct.numpy_classes(M, 2, 3, reverse=True)
    changed = int((rev[1].view(np.uint32) != want[1].view(np.uint32)).sum())
    print("score bit patterns changed by reversing the columns: %d of %d" % (changed, V))
    assert changed >= 1
    check(handle(bitlevel, D, packed).classes(2, 3, details=True), want)


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_dead_classes_and_negative_scores(handle, bitlevel):
    D = 65
    M, packed = model(bitlevel, D, 1000)
    # rows 0 and 1 are opposites and alone in class 2 of 3: it is dead, stays empty and attracts no row
    init = (np.arange(1000) % 2).astype(np.int32)
    init[:2] = 2
    ev = handle(bitlevel, D, packed)
    for iters in (1, 2, 10):
        got = ev.classes(3, iters, init=init, details=True)
        check(got, ct.host_classes(packed, D, bitlevel, 3, iters, init))
        assert not np.any(got[0] == 2) and got[3][2] == 0 and not np.any(got[2][2])
    # ten copies of a row and its negation at K = 1: the negation scores below 0 and still gets class 0, never a padded one
    Mn = np.concatenate([np.tile(M[5], (10, 1)), -M[5:6]]).astype(np.int8)
    pn = ct.pack(Mn, bitlevel)
    got = handle(bitlevel, D, pn).classes(1, 3, details=True)
    check(got, ct.host_classes(pn, D, bitlevel, 1, 3))
    assert np.all(got[0] == 0) and got[1][10] < 0 and np.all(got[1][:10] > 0)
    # every class dead: every row goes to class 0 with score +0
    Md = np.stack([M[3], M[4], -M[3], -M[4]]).astype(np.int8)
    pd = ct.pack(Md, bitlevel)
    got = handle(bitlevel, D, pd).classes(2, 5, details=True)
    check(got, ct.host_classes(pd, D, bitlevel, 2, 5))
    assert np.all(got[0] == 0) and np.all(got[1].view(np.uint32) == 0) and (got[4], got[5]) == (2, 0)


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_init_zero_iterations_and_refusals(handle, bitlevel, tmp_path):
    D, V, K = 200, 1000, 33
    M, packed = model(bitlevel, D, V)
    ev = handle(bitlevel, D, packed)
    init = np.random.default_rng(8).integers(0, K, V).astype(np.int32)
    check(ev.classes(K, 5, init=init, details=True), ct.host_classes(packed, D, bitlevel, K, 5, init))
    for start in (None, init):
        got = ev.classes(K, 0, init=start, details=True)
        check(got, ct.host_classes(packed, D, bitlevel, K, 0, start))
        assert np.all(got[1].view(np.uint32) == 0) and (got[4], got[5]) == (0, 0)
    L = _lib.lib()
    out = ct.outputs(V, D, K)

    def refused(why_part, h, k, iters, start):
        start = None if start is None else np.ascontiguousarray(start, np.int32)
        rc = L.w2b_eval_classes(h, k, iters, None if start is None else start.ctypes.data_as(_lib.i32p),
                                out[0].ctypes.data_as(_lib.i32p), out[1].ctypes.data_as(_lib.f32p), out[2].ctypes.data_as(_lib.i32p),
                                out[3].ctypes.data_as(_lib.i64p), out[4].ctypes.data_as(_lib.i32p), out[5].ctypes.data_as(_lib.i64p))
        why = L.w2b_last_error()
        assert rc == _lib.W2B_EINVAL and why_part in why, (rc, why)
        assert ct.untouched(out)

    for bad_k in (0, -3):
        refused(b"n_classes must be at least 1", ev._h, bad_k, 10, None)
        refused(b"n_classes must be at least 1", None, bad_k, 10, None)       # a NULL handle with a bad n_classes: the n_classes
    for bad_it in (-1, 1001):
        refused(b"max_iters must be 0..1000", ev._h, K, bad_it, None)
        refused(b"max_iters must be 0..1000", None, K, bad_it, None)
    refused(b"null handle", None, K, 10, None)
    refused(b"n_classes must be at most min(words, 16384)", ev._h, V + 1, 10, None)
    for row, bad in ((17, K), (3, -1)):
        bad_init = init.copy()
        bad_init[row] = bad
        bad_init[900] = K + 5
        refused(b"init: row %d: class out of range" % row, ev._h, K, 10, bad_init)
    lib = bits_testlib if bitlevel == 1 else codes_testlib
    f32 = w2b.Evaluator(write_vectors_file(str(tmp_path / "m.bin"), names(V), lib.values_of(M)), bitlevel, 0)
    try:
        refused(b"not available on an fp32 handle: load the file with bits or codes", f32._h, K, 10, None)
        with pytest.raises(w2b.W2bError) as e:
            f32.classes_text(K)
        assert e.value.code == _lib.W2B_EINVAL and "fp32 handle" in str(e.value)
    finally:
        f32.close()
    with pytest.raises(ValueError):
        ev.classes(K, init=init[:-1])


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_text_form_and_command_line(handle, bitlevel, tmp_path):
    D, V, K = 200, 1000, 33
    _, packed = model(bitlevel, D, V)
    mode = "bits" if bitlevel == 1 else "codes"
    ev = handle(bitlevel, D, packed)
    path = str(tmp_path / ("m%d_%d_%d.w2bp" % (bitlevel, D, V)))
    run = lambda *a: subprocess.run([CLASSES, *a], stdin=subprocess.DEVNULL, capture_output=True, timeout=300)
    for iters in (10, 2):
        want = ct.class_lines(names(V), twin(bitlevel, D, V, K, iters)[0])
        assert ev.classes_text(K, iters) == want
        r = run(path, str(K), str(iters), "0", mode)
        assert r.returncode == 0 and r.stdout == want, r.stderr
    assert ev.classes_text(K) == ct.class_lines(names(V), twin(bitlevel, D, V, K, 10)[0])          # iters defaults to 10
    r = run(path, str(K), mode)
    assert r.returncode == 0 and r.stdout == ev.classes_text(K), r.stderr
    # the threshold caps the rows, as it does for ./nearest
    capped = ct.host_classes(packed[:300], D, bitlevel, K, 10)[0]
    r = run(path, str(K), "10", "300", mode)
    assert r.returncode == 0 and r.stdout == ct.class_lines(names(300), capped), r.stderr
    assert np.array_equal(handle(bitlevel, D, packed, threshold=300).classes(K), capped)
    r = run(str(tmp_path / "no-such-file"), str(K), "10", "0", mode)
    assert r.stdout == b"Input file not found\n" and r.returncode == 255
    r = run(path, str(V + 1), "10", "0", mode)
    assert r.returncode == 1 and r.stdout == b"" and b"n_classes must be at most" in r.stderr


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_timing_counts_the_iterations_and_topk_is_unchanged(handle, bitlevel):
    D, V, K = 200, 1000, 65
    _, packed = model(bitlevel, D, V)
    ev = handle(bitlevel, D, packed)
    b = np.random.default_rng(3).integers(0, V, (3, 40)).astype(np.int32)
    before = ev.topk(*b, 10)
    ev.timing()
    it = ev.classes(K, 6, details=True)[4]
    ms, launches, macs = ev.timing()
    assert launches == it and ms > 0 and macs == float(it) * K * V * D
    a_ms, s_ms = ev.classes_timing()
    assert a_ms > 0 and s_ms > 0 and abs(a_ms + s_ms - ms) <= 1e-6 * ms
    ev.classes(K, 0)
    ms, launches, macs = ev.timing()
    assert launches == 0 and macs == 0.0 and ms > 0 and ev.classes_timing()[0] == 0.0      # the sums pass alone
    assert ev.timing() == (0.0, 0, 0.0)
    after = ev.topk(*b, 10)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
