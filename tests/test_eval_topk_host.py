"""Top-k evaluator, the part that needs no GPU: the checker of tests/test_gpu_eval_topk.py (k rounds of the pinned
top-1 oracle) against a literal transcription of the reference's insertion loop, the new ABI, and ./nearest's argument
handling before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from word2bits_amd import _lib
from w2b_testlib import ROOT, eval_oracle, write_vectors_file
from topk_testlib import insertion_topk, oracle_topk, seeded_matrix

CLI = os.path.join(ROOT, "nearest")
SYMBOLS = ["w2b_eval_topk", "w2b_eval_neighbors", "w2b_eval_nearest_text", "w2b_eval_set_topk_scratch"]


@pytest.mark.parametrize("kind,V,D,k,Q", [("1bit", 3000, 200, 10, 12), ("1bit", 40, 5, 64, 40), ("fp", 500, 30, 10, 12)])
def test_iterated_oracle_equals_the_insertion_loop(kind, V, D, k, Q, tmp_path):
    E = eval_oracle()
    rng = np.random.default_rng(V + D)
    M = seeded_matrix(rng, kind, V, D)
    if kind == "fp":
        M[7] = 0                                      # a zero row: NaN after the normalisation, never in a list
    path = write_vectors_file(str(tmp_path / "v.bin"), [b"w%d" % i for i in range(V)], M)
    om = E.EvalModel(path, 0, 0, fma=False)
    b = rng.integers(0, V, (3, Q)).astype(np.int32)
    b[:, :3] = b[0, :3]                               # b1 == b2 == b3
    rows, scores = oracle_topk(om, *b, k)
    short = 0
    for q in range(Q):
        wr, wd = insertion_topk(om.M, b[0, q], b[1, q], b[2, q], k)
        assert np.array_equal(rows[q], wr), q
        assert np.array_equal(scores[q].view(np.uint32), wd.view(np.uint32)), q
        short += int(wr[-1] < 0)
    if V == 40:
        assert short == Q                             # fewer than k rows qualify: -1 / 0 tails everywhere


def test_abi_is_exported_declared_and_documented():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib._PROTOTYPES if hasattr(_lib, "_PROTOTYPES") else name in open(_lib.__file__).read(), name
    header = open(os.path.join(ROOT, "include", "word2bits_eval.h")).read()
    assert re.search(r"#define\s+W2B_EVAL_MAX_K\s+64\b", header)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % name, header), name


def test_nearest_usage_and_k_range(tmp_path):
    r = subprocess.run([CLI], capture_output=True)
    assert r.returncode == 0 and r.stdout.startswith(b"Usage: ./nearest <FILE> <k>")
    path = write_vectors_file(str(tmp_path / "v.bin"), [b"a", b"b"], np.eye(2, dtype=np.float32))
    for k in ("0", "65"):
        r = subprocess.run([CLI, path, k], capture_output=True, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"" and b"k must be 1..64" in r.stderr
