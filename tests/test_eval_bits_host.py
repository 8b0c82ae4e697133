"""Bits-mode evaluator (include/word2bits_eval.h, "bits mode"), the part that needs no GPU: the new ABI, the host twin of
the kernels against the numpy definition, the agreement of the integer ranking with the pinned float oracle that lets
tests/test_gpu_eval_bits.py use the integer definition as the truth, and the command lines' handling of `bits` before
they touch a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from word2bits_amd import _lib
from w2b_testlib import GOLDEN, ROOT, eval_oracle, write_vectors_file
from bits_testlib import (int_scores, make_signs, oracle_chain_scores, pack_signs, signs_of_bits, values_of,
                          write_packed_file)

SYMBOLS = ["w2b_eval_load_bits", "w2b_eval_bits_from_trainer", "w2b_eval_get_bits", "w2b_bits_scores_host"]


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_eval.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\(" % name, header), name
    assert hasattr(lib, "w2b_eval_is_bits") and "w2b_eval_is_bits" in _lib.SIGNATURES
    assert re.search(r"\bint32_t\s+w2b_eval_is_bits\(", header)


def host_scores(packed, D, b1, b2, b3):
    out = np.empty(packed.shape[0], np.int32)
    _lib.check(_lib.lib().w2b_bits_scores_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0], D, int(b1), int(b2),
                                               int(b3), out.ctypes.data_as(_lib.i32p)))
    return out


@pytest.mark.parametrize("D", [1, 7, 37, 63, 64, 65, 200, 1000])
@pytest.mark.parametrize("kind", ["random", "corr"])
def test_host_twin_equals_the_numpy_definition(D, kind):
    rng = np.random.default_rng(1000 + D)
    V, Q = 300, 24
    S = make_signs(rng, kind, V, D)
    packed = pack_signs(S)                                   # through w2b_pack_quantized: the file's layout
    assert packed.shape == (V, (D + 63) // 64) and np.array_equal(signs_of_bits(packed, D), S)
    b = rng.integers(0, V, (3, Q))
    b[:, :6] = b[0, :6]                                      # b1 == b2 == b3: D - 2 * Hamming
    want = (S[b[1]].astype(np.int64) - S[b[0]] + S[b[2]]) @ S.T.astype(np.int64)
    assert np.array_equal(int_scores(S, *b), want)           # the test library's own fast form
    for q in range(Q):
        assert np.array_equal(host_scores(packed, D, *b[:, q]), want[q]), q
    r = int(b[0, 0])
    ham = (S != S[r]).sum(1)
    assert np.array_equal(host_scores(packed, D, r, r, r), D - 2 * ham)
    L = _lib.lib()
    bad = np.empty(V, np.int32)
    assert L.w2b_bits_scores_host(packed.ctypes.data_as(_lib.u64p), V, D, V, 0, 0, bad.ctypes.data_as(_lib.i32p)) == _lib.W2B_EINVAL


def agreement(om, fma, b, label):
    """Every statement under "Why" of the bits mode, for the questions b = (b1, b2, b3) on the EvalModel `om`."""
    D = om.size
    S = np.where(om.M < 0, -1, 1).astype(np.int8)
    assert np.all(np.abs(np.abs(om.M) * np.sqrt(np.float32(D)) - 1) < 1e-3)     # a 1-bit model: every |value| = 1/sqrt(D)
    I = int_scores(S, *b)
    F = oracle_chain_scores(om.M, *b, fma)
    best, bestd = om.top1(*(x.astype(np.int32) for x in b))
    worst = 0.0
    for q in range(len(b[0])):
        f, i = F[q], I[q]
        # the numpy chain is the pinned oracle's: its strict-greater arg-max over the allowed rows is the oracle's answer
        allowed = np.ones(om.words, bool)
        allowed[[b[0][q], b[1][q], b[2][q]]] = False
        fa = np.where(allowed & (f > 0), f, np.float32(0))
        if fa.max() > 0:
            assert best[q] == int(np.argmax(fa)) and bestd[q].view(np.uint32) == fa.max().view(np.uint32), (label, q)
        else:
            assert best[q] == -1, (label, q)
        # I(c) > I(c') implies score(c) > score(c'), for every pair of rows: consecutive levels of I do not overlap
        levels = np.unique(i)
        order = np.argsort(i, kind="stable")
        cuts = np.searchsorted(i[order], levels)
        lo = np.minimum.reduceat(f[order], cuts)
        hi = np.maximum.reduceat(f[order], cuts)
        assert np.all(hi[:-1] < lo[1:]), (label, q)
        assert np.all(f[i > 0] > 0), (label, q)
        # the oracle's top-1 row has the maximal I whenever that maximum is > 0
        imax = i[allowed].max() if allowed.any() else 0
        if imax > 0:
            assert best[q] >= 0 and i[best[q]] == imax, (label, q)
        worst = max(worst, float(np.abs(f.astype(np.float64) - i / D).max()))
    # derived: the normalised value m = fl(1/3 / fl(sqrt(fl(D/9)))) is 1/sqrt(D) within 3 roundings, vec within 1 more, and the
    # chain adds one rounding (of a partial sum of magnitude <= 3) per step: |score - I/D| <= 3 (D + 3) 2^-24
    bound = 3 * (D + 3) * 2.0 ** -24
    print("%s fma=%d D=%d: max |score - I/D| = %.3g, bound %.3g, half step %.3g" % (label, fma, D, worst, bound, 1 / D))
    assert worst <= bound < 1 / D / 5.5


@pytest.mark.parametrize("fma", [True, False])
def test_integer_ranking_agrees_with_the_float_oracle_on_the_fixture(fma):
    E = eval_oracle()
    om = E.EvalModel(os.path.join(GOLDEN, "eval_1bit.bin"), 0, 0, fma=fma)
    rng = np.random.default_rng(2)
    b = rng.integers(0, om.words, (3, 60))
    b[:, :5] = b[0, :5]
    agreement(om, fma, b, "eval_1bit.bin")


@pytest.mark.parametrize("fma", [True, False])
@pytest.mark.parametrize("D,V,Q", [(7, 3000, 40), (37, 3000, 40), (64, 3000, 40), (200, 3000, 40), (300, 3000, 40),
                                   (1000, 1500, 16)])
def test_integer_ranking_agrees_with_the_float_oracle_on_seeded_files(D, V, Q, fma, tmp_path):
    E = eval_oracle()
    rng = np.random.default_rng(D)
    S = make_signs(rng, "corr" if D % 2 == 0 else "random", V, D)
    path = write_vectors_file(str(tmp_path / "v.bin"), [b"w%d" % i for i in range(V)], values_of(S))
    om = E.EvalModel(path, 0, 0, fma=fma)
    b = rng.integers(0, V, (3, Q))
    b[:, :4] = b[0, :4]
    agreement(om, fma, b, "seeded")


def test_command_lines_handle_bits_before_a_device_is_touched(tmp_path):
    acc, near = os.path.join(ROOT, "compute_accuracy"), os.path.join(ROOT, "nearest")
    r = subprocess.run([acc], capture_output=True)
    assert r.returncode == 0 and r.stdout.startswith(b"Usage: ./compute-accuracy <FILE> <bitlevel> <threshold>\n")
    assert b"bits" not in r.stdout and b"bits" in r.stderr            # the reference's usage text stays what it was
    r = subprocess.run([near], capture_output=True)
    assert r.returncode == 0 and r.stdout.startswith(b"Usage: ./nearest <FILE> <k>") and b"fma|nofma|bits" in r.stdout
    S = make_signs(np.random.default_rng(0), "random", 2, 5)
    pk = write_packed_file(str(tmp_path / "v.w2bp"), [b"a", b"b"], pack_signs(S), 5)
    for k in ("0", "65"):
        r = subprocess.run([near, pk, k, "0", "0", "bits"], capture_output=True, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"" and b"k must be 1..64" in r.stderr
    missing = str(tmp_path / "missing.w2bp")
    for cmd in ([acc, missing, "0", "0", "bits"], [near, missing, "3", "0", "0", "bits"]):
        r = subprocess.run(cmd, capture_output=True, stdin=subprocess.DEVNULL)
        assert r.stdout == b"Input file not found\n" and r.returncode == 255
    # a 2-bit packed model has no integer ranking: refused while the file is read
    two = str(tmp_path / "two.w2bp")
    with open(two, "wb") as f:
        f.write(b"W2BP1 2 5 2\na\nb\n" + np.zeros(4, "<u8").tobytes())
    for cmd in ([acc, two, "0", "0", "bits"], [near, two, "3", "0", "0", "bits"]):
        r = subprocess.run(cmd, capture_output=True, stdin=subprocess.DEVNULL)
        assert r.returncode == 1 and r.stdout == b"" and b"2-bit" in r.stderr
