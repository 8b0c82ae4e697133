"""Packed embedding layer (include/word2bits_embed.h), the part that needs no GPU: the ABI, the host twins of the kernels
against a numpy definition written here (unpack through w2b_unpack_quantized, int64 sums, the stated float32 steps; bit
for bit), the validation of the host form, and what w2b_embed_load reports before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT

SYMBOLS = {
    "w2b_embed_load": "int", "w2b_embed_create": "int", "w2b_embed_free": "void", "w2b_embed_rows": "int64_t",
    "w2b_embed_dim": "int64_t", "w2b_embed_bitlevel": "int32_t", "w2b_embed_word": r"const char \*",
    "w2b_embed_search": "int64_t", "w2b_embed_lookup": "int", "w2b_embed_bag": "int", "w2b_embed_reserve": "int",
    "w2b_embed_lookup_device": "int", "w2b_embed_bag_device": "int", "w2b_embed_synchronize": "int",
    "w2b_embed_bad_ids": "int", "w2b_embed_timing_read": "int", "w2b_embed_lookup_host": "int", "w2b_embed_bag_host": "int",
}
MAX_BAG = 1 << 22
Q1 = np.array([0x3EAAAAAB], np.uint32).view(np.float32)[0]


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_embed.h")).read()
    for name, res in SYMBOLS.items():
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"^%s\s*%s\(" % (res, name), header, flags=re.M), name
    for const, val in (("W2B_EMBED_F32", "0"), ("W2B_EMBED_BF16", "1"), ("W2B_EMBED_F16", "2"), ("W2B_EMBED_SUM", "0"),
                       ("W2B_EMBED_MEAN", "1"), ("W2B_EMBED_MAX_BAG", "(1 << 22)")):
        assert re.search(r"^#define %s %s$" % (const, re.escape(val)), header, flags=re.M), const
    assert hasattr(w2b, "PackedEmbedding")


# ------------------------------------------------------------------------------------------ the definition, in numpy
def make_table(rng, rows, dim, bitlevel):
    """(packed uint64 [rows, wpr], unpacked float32 [rows, dim]) of a random quantized table"""
    mags = np.array([Q1] if bitlevel == 1 else [0.25, 0.75], np.float32)
    vals = (rng.choice(mags, (rows, dim)) * rng.choice(np.array([-1, 1], np.float32), (rows, dim))).astype(np.float32)
    packed = w2b.pack_quantized(vals, bitlevel)
    table = w2b.unpack_quantized(packed, dim, bitlevel)              # through w2b_unpack_quantized
    assert np.array_equal(table.view(np.uint32), vals.view(np.uint32))
    return packed, table


def ref_lookup(table, ids):
    out = table[np.maximum(ids, 0)].copy()
    out[ids < 0] = 0.0
    return out


def ref_bag(table, bitlevel, ids, offsets, mode):
    """T by int64 sums of the integer codes, then the float32 steps of the header"""
    q = Q1 if bitlevel == 1 else np.float32(0.25)
    codes = np.rint(table.astype(np.float64) / np.float64(q)).astype(np.int64)     # +-1 | +-1, +-3: exact
    assert set(np.unique(codes).tolist()) <= ({-1, 1} if bitlevel == 1 else {-3, -1, 1, 3})
    out = np.zeros((len(offsets) - 1, table.shape[1]), np.float32)
    for b in range(len(offsets) - 1):
        sel = ids[offsets[b]:offsets[b + 1]]
        sel = sel[sel >= 0]
        T = codes[sel].sum(axis=0, dtype=np.int64)
        s = T.astype(np.float32) * q
        if mode == "mean":
            s = s / np.float32(len(sel)) if len(sel) else np.zeros_like(s)
        out[b] = s
    return out


def make_ids_and_bags(rng, rows, long_bag=5000):
    """ids with repeats and negatives; bags: empty, padding only, single id, the first and the last id of the array, and
    one long bag"""
    parts = [rng.integers(0, rows, 7), [], np.full(4, -1), [rows - 1], rng.integers(-1, rows, long_bag),
             rng.integers(0, rows, 3), [], [0, 0, 5 % rows, -1, 0], rng.integers(-2, rows, 40)]
    ids = np.concatenate([np.asarray(p, np.int64) for p in parts]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return ids, offsets


def host_lookup(packed, dim, bitlevel, ids):
    out = np.full((len(ids), dim), np.nan, np.float32)
    rc = _lib.lib().w2b_embed_lookup_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0], dim, bitlevel, len(ids),
                                          ids.ctypes.data_as(_lib.i32p), out.ctypes.data_as(_lib.f32p))
    return rc, out


def host_bag(packed, dim, bitlevel, ids, offsets, mode, n_bags=None, n_ids=None):
    n_bags = len(offsets) - 1 if n_bags is None else n_bags
    out = np.full((max(n_bags, 0), dim), np.nan, np.float32)
    rc = _lib.lib().w2b_embed_bag_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0], dim, bitlevel,
                                       len(ids) if n_ids is None else n_ids, ids.ctypes.data_as(_lib.i32p), n_bags,
                                       offsets.ctypes.data_as(_lib.i64p), mode, out.ctypes.data_as(_lib.f32p))
    return rc, out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 3, 63, 64, 65, 200])
def test_host_twins_equal_the_numpy_definition(dim, bitlevel):
    rng = np.random.default_rng(100 * dim + bitlevel)
    rows = 300
    packed, table = make_table(rng, rows, dim, bitlevel)
    ids, offsets = make_ids_and_bags(rng, rows)
    assert (ids < 0).any() and len(np.unique(ids)) < len(ids) and np.diff(offsets).max() == 5000
    rc, got = host_lookup(packed, dim, bitlevel, ids)
    assert rc == 0 and same_bits(got, ref_lookup(table, ids))
    assert not np.signbit(got[ids < 0]).any()                              # padding rows are +0.0
    pats = set(np.unique(got[ids >= 0].view(np.uint32)).tolist())
    assert pats <= ({0x3EAAAAAB, 0xBEAAAAAB} if bitlevel == 1 else {0x3E800000, 0xBE800000, 0x3F400000, 0xBF400000})
    for code, mode in enumerate(("sum", "mean")):
        rc, got = host_bag(packed, dim, bitlevel, ids, offsets, code)
        want = ref_bag(table, bitlevel, ids, offsets, mode)
        assert rc == 0 and same_bits(got, want), mode
        assert np.all(got[1].view(np.uint32) == 0) and np.all(got[2].view(np.uint32) == 0)    # empty / padding only: +0.0
        assert same_bits(got[3], table[rows - 1])                           # a single id: the row itself, sum and mean
    if bitlevel == 2:                                                      # multiples of .25 add exactly in float32
        rc, got = host_bag(packed, dim, bitlevel, ids, offsets, 0)
        seq = np.zeros_like(got)
        for b in range(len(offsets) - 1):
            for r in ids[offsets[b]:offsets[b + 1]]:
                if r >= 0:
                    seq[b] += table[r]
        assert same_bits(got, seq + np.float32(0.0))


def test_validation_of_ids_offsets_mode_and_bitlevel():
    rng = np.random.default_rng(5)
    rows, dim = 300, 65
    packed, _ = make_table(rng, rows, dim, 2)
    L = _lib.lib()
    err = lambda: L.w2b_last_error().decode()
    ids = np.array([1, 2, rows, 3], np.int32)
    rc, out = host_lookup(packed, dim, 2, ids)
    assert rc == _lib.W2B_EINVAL and "rows" in err() and np.isnan(out).all()             # nothing written
    good = np.array([1, 2, -1, 3], np.int32)
    off = lambda *x: np.array(x, np.int64)
    rc, out = host_bag(packed, dim, 2, ids, off(0, 2, 4), 0)
    assert rc == _lib.W2B_EINVAL and "rows" in err() and np.isnan(out).all()
    rc, _ = host_bag(packed, dim, 2, good, off(0, 3, 2, 4), 0)
    assert rc == _lib.W2B_EINVAL and "decrease" in err()
    rc, _ = host_bag(packed, dim, 2, good, off(1, 2, 4), 0)
    assert rc == _lib.W2B_EINVAL and "offsets[0]" in err()
    rc, _ = host_bag(packed, dim, 2, good, off(0, 2, 3), 0)
    assert rc == _lib.W2B_EINVAL and "offsets[n_bags]" in err()
    rc, _ = host_bag(packed, dim, 2, good, off(0, 2, 4), 2)
    assert rc == _lib.W2B_EINVAL and "mode" in err()
    rc, _ = host_bag(packed, dim, 2, good, off(0, 2, 4), 0, n_bags=-1)
    assert rc == _lib.W2B_EINVAL
    assert L.w2b_embed_lookup_host(packed.ctypes.data_as(_lib.u64p), rows, dim, 2, -1, good.ctypes.data_as(_lib.i32p),
                                   None) == _lib.W2B_EINVAL
    pad = np.full(MAX_BAG + 1, -1, np.int32)                                # one bag of padding, one id too long
    rc, _ = host_bag(packed, 1, 2, pad, off(0, MAX_BAG + 1), 1)
    assert rc == _lib.W2B_EINVAL and "W2B_EMBED_MAX_BAG" in err()
    rc, out = host_bag(packed, 1, 2, pad[:MAX_BAG], off(0, MAX_BAG), 1)     # the cap itself is fine: m == 0, +0.0
    assert rc == 0 and out.view(np.uint32)[0, 0] == 0
    rc, _ = host_lookup(packed, dim, 3, good)
    assert rc == _lib.W2B_EUNSUPPORTED
    rc, _ = host_bag(packed, dim, 3, good, off(0, 2, 4), 0)
    assert rc == _lib.W2B_EUNSUPPORTED
    h = C.c_void_p()
    assert L.w2b_embed_create(packed.ctypes.data_as(_lib.u64p), rows, dim, 3, 0, C.byref(h)) == _lib.W2B_EUNSUPPORTED
    rc, out = host_lookup(packed, dim, 2, np.zeros(0, np.int32))            # n == 0
    assert rc == 0
    rc, out = host_bag(packed, dim, 2, np.zeros(0, np.int32), off(0), 0)    # n_bags == 0
    assert rc == 0


def test_load_reports_file_errors_before_it_asks_for_a_device(tmp_path):
    """a missing file and a float file fail the same way whether or not a GPU is visible"""
    L = _lib.lib()
    h = C.c_void_p()
    assert L.w2b_embed_load(str(tmp_path / "absent.w2bp").encode(), 0, 0, C.byref(h)) == _lib.W2B_EIO
    assert L.w2b_last_error() == b"Input file not found" and not h
    path = str(tmp_path / "float.bin")                                      # the reference's binary format
    with open(path, "wb") as f:
        f.write(b"2 3\n")
        for w in (b"a", b"b"):
            f.write(w + b" " + np.array([0.25, -0.25, 0.75], np.float32).tobytes() + b"\n")
    assert L.w2b_embed_load(path.encode(), 0, 0, C.byref(h)) == _lib.W2B_EINVAL
    assert b"W2BP1" in L.w2b_last_error() and not h
    with pytest.raises(w2b.W2bError) as e:
        w2b.PackedEmbedding(path)
    assert e.value.code == _lib.W2B_EINVAL


def test_the_twins_run_clean_under_the_host_sanitizers():
    """tests/host/embed_bag_twin_main.cpp with w2b_embed_twins.cpp, built with -fsanitize=address,undefined as a program of
    its own (the Makefile's host-check target for it) and run once: no library, no Python, no GPU under the sanitizer"""
    csrc = os.path.join(ROOT, "word2bits_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "build/embed_bag_twin_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(csrc, "build", "embed_bag_twin_check")], capture_output=True, text=True,
                       stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    for name in ("w2b_embed_lookup_host", "w2b_embed_bag_host", "w2b_embed_bag_weighted_host"):
        assert re.search(r"^%s: \d+ calls ok, \d+ refused$" % name, r.stdout, flags=re.M), r.stdout + r.stderr
