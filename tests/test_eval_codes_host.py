"""Codes-mode evaluator (include/word2bits_eval.h, "codes mode"), the part that needs no GPU: the new ABI, the host twin of
the kernels against the numpy definition (bit-identical), packing, the agreement of the ranking with the pinned float
oracle within the derived rounding bound, and the command lines' handling of `codes` before they touch a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT, eval_oracle, write_vectors_file
from bits_testlib import oracle_chain_scores, make_signs, pack_signs
from bits_testlib import write_packed_file as write_packed_file_1bit
from codes_testlib import (codes_of_packed, float_bound, int_products, lead_over_runner_up, make_codes, pack_codes, scores,
                           values_of, weights, write_packed_file)

SYMBOLS = ["w2b_eval_load_codes", "w2b_eval_codes_from_trainer", "w2b_eval_get_codes", "w2b_codes_scores_host"]


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_eval.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\(" % name, header), name
    assert hasattr(lib, "w2b_eval_is_codes") and "w2b_eval_is_codes" in _lib.SIGNATURES
    assert re.search(r"\bint32_t\s+w2b_eval_is_codes\(", header)
    assert "out of scope" not in header


def host_scores(packed, D, b1, b2, b3):
    V = packed.shape[0]
    J, s = np.empty((3, V), np.int32), np.empty(V, np.float32)
    _lib.check(_lib.lib().w2b_codes_scores_host(packed.ctypes.data_as(_lib.u64p), V, D, int(b1), int(b2), int(b3),
                                                J.ctypes.data_as(_lib.i32p), s.ctypes.data_as(_lib.f32p)))
    return J, s


@pytest.mark.parametrize("D", [1, 7, 31, 32, 33, 37, 64, 65, 200, 1000])
@pytest.mark.parametrize("kind", ["random", "corr"])
def test_host_twin_equals_the_numpy_definition(D, kind):
    rng = np.random.default_rng(2000 + D)
    V, Q = 300, 24
    T = make_codes(rng, kind, V, D)
    packed = pack_codes(T)                                   # through w2b_pack_quantized: the file's layout
    assert packed.shape == (V, 2 * ((D + 63) // 64)) and np.array_equal(codes_of_packed(packed, D), T)
    b = rng.integers(0, V, (3, Q))
    b[:, :6] = b[0, :6]                                      # b1 == b2 == b3
    want_J = [T[b[i]].astype(np.int64) @ T.T.astype(np.int64) for i in range(3)]
    for i in range(3):
        assert np.array_equal(int_products(T, b[i]), want_J[i])          # the test library's own fast form
    S = scores(T, *b)
    for q in range(Q):
        J, s = host_scores(packed, D, *b[:, q])
        for i in range(3):
            assert np.array_equal(J[i], want_J[i][q]), (q, i)
        assert np.array_equal(s.view(np.uint32), S[q].view(np.uint32)), q
    w = weights(T)
    r = int(b[0, 0])
    _, s = host_scores(packed, D, r, r, r)                   # reduces to (J w(r)) w(c)
    want = (int_products(T, [r])[0].astype(np.float32) * w[r]) * w
    assert np.array_equal(s.view(np.uint32), want.view(np.uint32))
    L = _lib.lib()
    for bad in ((V, 0, 0), (0, -1, 0), (0, 0, V)):
        assert L.w2b_codes_scores_host(packed.ctypes.data_as(_lib.u64p), V, D, *bad, None, s.ctypes.data_as(_lib.f32p)) == _lib.W2B_EINVAL
    assert L.w2b_codes_scores_host(packed.ctypes.data_as(_lib.u64p), V, D, 0, 1, 2, None, None) == _lib.W2B_OK


def test_packing_of_a_seeded_quantized_model():
    rng = np.random.default_rng(5)
    V, D = 50, 130
    T = make_codes(rng, "random", V, D)
    packed = w2b.pack_quantized(values_of(T), 2)
    nb = (D + 63) // 64
    assert packed.shape == (V, 2 * nb)
    for r in (0, 17, 49):
        for c in (0, 63, 64, 129):
            assert (int(packed[r, 2 * (c // 64)]) >> (c % 64)) & 1 == int(T[r, c] < 0)
            assert (int(packed[r, 2 * (c // 64) + 1]) >> (c % 64)) & 1 == int(abs(T[r, c]) == 3)
    assert np.all(packed[:, 2 * nb - 2:] >> np.uint64(D - 64 * (nb - 1)) == 0)           # padding bits are zero
    assert np.array_equal(codes_of_packed(packed, D), T)


@pytest.mark.parametrize("fma", [True, False])
@pytest.mark.parametrize("D,V,Q", [(37, 2000, 40), (200, 2000, 40), (400, 1500, 24)])
def test_ranking_agrees_with_the_float_oracle_on_seeded_files(D, V, Q, fma, tmp_path):
    E = eval_oracle()
    rng = np.random.default_rng(D)
    T = make_codes(rng, "corr" if D == 200 else "random", V, D)
    path = write_vectors_file(str(tmp_path / "v.bin"), [b"w%d" % i for i in range(V)], values_of(T))
    om = E.EvalModel(path, 2, 0, fma=fma)
    b = rng.integers(0, V, (3, Q))
    b[:, :4] = b[0, :4]
    packed = pack_codes(T)
    S = np.stack([host_scores(packed, D, *b[:, q])[1] for q in range(Q)])                # the host twin
    assert np.array_equal(S.view(np.uint32), scores(T, *b).view(np.uint32))
    F = oracle_chain_scores(om.M, *b, fma)
    best, bestd = om.top1(*(x.astype(np.int32) for x in b))
    bound = float_bound(D)
    lead = lead_over_runner_up(S, *b)
    worst, skipped = 0.0, 0
    for q in range(Q):
        f, s = F[q], S[q]
        allowed = np.ones(V, bool)
        allowed[[b[0][q], b[1][q], b[2][q]]] = False
        # the numpy chain is the pinned oracle's: its strict-greater arg-max over the allowed rows is the oracle's answer
        fa = np.where(allowed & (f > 0), f, np.float32(0))
        if fa.max() > 0:
            assert best[q] == int(np.argmax(fa)) and bestd[q].view(np.uint32) == fa.max().view(np.uint32), q
        else:
            assert best[q] == -1, q
        worst = max(worst, float(np.abs(f.astype(np.float64) - s.astype(np.float64)).max()))
        # rows whose codes scores differ by more than 2 x bound are never ordered the other way by the oracle
        order = np.argsort(s, kind="stable")
        ss, fs = s[order].astype(np.float64), f[order].astype(np.float64)
        below = np.searchsorted(ss, ss - 2 * bound, side="left")          # rows [0, below) score less by more than 2 x bound
        pmax = np.concatenate([[-np.inf], np.maximum.accumulate(fs)])
        assert np.all(fs > pmax[below]), q
        # the oracle's top-1 is the codes top-1 whenever that one leads its runner-up by more than 2 x bound
        if lead[q] > 2 * bound:
            sa = np.where(allowed, s, np.float32(0))
            assert best[q] == int(np.argmax(sa)), q
        else:
            skipped += 1
    print("fma=%d D=%d: max |fp32 chain - codes| = %.3g, bound %.3g; top-1 comparison skipped for %d of %d questions"
          % (fma, D, worst, bound, skipped, Q))
    assert worst <= bound
    assert skipped < Q / 2


def test_both_packed_modes_at_once_are_refused(tmp_path):
    with pytest.raises(ValueError):
        w2b.Evaluator(str(tmp_path / "x.w2bp"), bits=True, codes=True)
    with pytest.raises(ValueError):
        w2b.Evaluator.from_trainer(None, [], bits=True, codes=True)


def test_command_lines_handle_codes_before_a_device_is_touched(tmp_path):
    acc, near = os.path.join(ROOT, "compute_accuracy"), os.path.join(ROOT, "nearest")
    r = subprocess.run([acc], capture_output=True)
    assert r.returncode == 0 and r.stdout.startswith(b"Usage: ./compute-accuracy <FILE> <bitlevel> <threshold>\n")
    assert b"codes" not in r.stdout and b"codes" in r.stderr          # the reference's usage text stays what it was
    r = subprocess.run([near], capture_output=True)
    assert r.returncode == 0 and b"fma|nofma|bits" in r.stdout and b"codes" in r.stdout
    T = make_codes(np.random.default_rng(0), "random", 2, 5)
    pk = write_packed_file(str(tmp_path / "v.w2bp"), [b"a", b"b"], pack_codes(T), 5)
    for k in ("0", "65"):
        r = subprocess.run([near, pk, k, "0", "0", "codes"], capture_output=True, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"" and b"k must be 1..64" in r.stderr
    missing = str(tmp_path / "missing.w2bp")
    for cmd in ([acc, missing, "0", "0", "codes"], [near, missing, "3", "0", "0", "codes"]):
        r = subprocess.run(cmd, capture_output=True, stdin=subprocess.DEVNULL)
        assert r.stdout == b"Input file not found\n" and r.returncode == 255
    one = write_packed_file_1bit(str(tmp_path / "one.w2bp"), [b"a", b"b"], pack_signs(make_signs(np.random.default_rng(0), "random", 2, 5)), 5)
    for cmd in ([acc, one, "0", "0", "codes"], [near, one, "3", "0", "0", "codes"]):
        r = subprocess.run(cmd, capture_output=True, stdin=subprocess.DEVNULL)
        assert r.returncode == 1 and r.stdout == b"" and b"bits" in r.stderr
