"""Weighted bag pooling of the packed embedding layer (include/word2bits_embed.h, "Weighted bag"), the part that needs no
GPU: the ABI, the host twin against a numpy definition written here (one float32 fused multiply-add per id, segments of
W2B_EMBED_WSEG positions, bit for bit), the identities the header states, and the validation of the weights."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from word2bits_amd import _lib
from w2b_testlib import ROOT
from test_embed_host import Q1, host_bag, make_table, same_bits

SYMBOLS = ("w2b_embed_bag_weighted", "w2b_embed_reserve_weights", "w2b_embed_bag_weighted_device",
           "w2b_embed_bag_weighted_host")
WSEG = 1024
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049, 2500]
ROWS = 300


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_embed.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int, name
        assert re.search(r"^int\s*%s\(" % name, header, flags=re.M), name
    assert re.search(r"^#define W2B_EMBED_WSEG 1024$", header, flags=re.M)


# ------------------------------------------------------------------------------------------ the definition, in numpy
def codes_of(table, bitlevel):
    q = Q1 if bitlevel == 1 else np.float32(0.25)
    codes = np.rint(table.astype(np.float64) / np.float64(q))              # +-1 | +-1, +-3: exact
    assert set(np.unique(codes).tolist()) <= ({-1, 1} if bitlevel == 1 else {-3, -1, 1, 3})
    return codes


def chain(codes, ids, weights, acc=None):
    """acc = fmaf(w_i, t_i, acc) over the ids >= 0 in order, per column, in float32.  With weights k / 64, |k| < 2^20, and
    at most 5000 ids every product and partial sum is a multiple of 2^-6 below 2^36: float64(acc) + float64(w) * t is
    exact, and rounding it to float32 once is the fused multiply-add."""
    acc = np.zeros(codes.shape[1], np.float32) if acc is None else acc
    for r, w in zip(ids, weights):
        if r >= 0:
            acc = (acc.astype(np.float64) + np.float64(w) * codes[r]).astype(np.float32)
    return acc


def finish(S, m, bitlevel, mode):
    q = Q1 if bitlevel == 1 else np.float32(0.25)
    s = S.astype(np.float32) * q
    if mode == "mean":
        s = s / np.float32(m) if m else np.zeros_like(s)
    return s


def ref_weighted(codes, bitlevel, ids, weights, offsets, mode, seg=WSEG):
    out = np.zeros((len(offsets) - 1, codes.shape[1]), np.float32)
    for b in range(len(offsets) - 1):
        S = np.zeros(codes.shape[1], np.float32)
        for s0 in range(offsets[b], offsets[b + 1], seg):
            s1 = min(s0 + seg, offsets[b + 1])
            S = S + chain(codes, ids[s0:s1], weights[s0:s1])                # float32 + float32: one rounded add
        out[b] = finish(S, int((ids[offsets[b]:offsets[b + 1]] >= 0).sum()), bitlevel, mode)
    return out


def make_bags(rng, rows, lengths=LENGTHS, extra=()):
    """bags of the given lengths in a shuffled order, then an all-padding bag and one with repeats and padding; the ids of
    the longer bags hold some padding too"""
    lens = list(lengths) + list(extra)
    rng.shuffle(lens)
    parts = [rng.integers(-1 if n > 5 else 0, rows, n) for n in lens]
    parts += [np.full(6, -1), [0, 0, 5 % rows, -1, 0, rows - 1, 0]]
    ids = np.concatenate([np.asarray(p, np.int64) for p in parts]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return ids, offsets


def dyadic_weights(rng, n, kmax=(1 << 20) - 1):
    """k / 64 with integer |k| <= kmax; exact in float32"""
    return (rng.integers(-kmax, kmax + 1, n).astype(np.float64) / 64.0).astype(np.float32)


def host_bag_weighted(packed, dim, bitlevel, ids, weights, offsets, mode, null_weights=False):
    n_bags = len(offsets) - 1
    out = np.full((max(n_bags, 0), dim), np.nan, np.float32)
    wp = None if null_weights else weights.ctypes.data_as(_lib.f32p)
    rc = _lib.lib().w2b_embed_bag_weighted_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0], dim, bitlevel, len(ids),
                                                ids.ctypes.data_as(_lib.i32p), wp, n_bags,
                                                offsets.ctypes.data_as(_lib.i64p), mode, out.ctypes.data_as(_lib.f32p))
    return rc, out


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 3, 64, 65, 200])
def test_twin_equals_the_numpy_definition(dim, bitlevel):
    rng = np.random.default_rng(1000 * dim + bitlevel)
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    codes = codes_of(table, bitlevel)
    ids, offsets = make_bags(rng, ROWS)
    weights = dyadic_weights(rng, len(ids))
    weights[::97] = 0.0
    assert (ids < 0).any() and len(np.unique(ids)) < len(ids) and np.diff(offsets).max() == 2500
    for code, mode in enumerate(("sum", "mean")):
        rc, got = host_bag_weighted(packed, dim, bitlevel, ids, weights, offsets, code)
        assert rc == 0 and same_bits(got, ref_weighted(codes, bitlevel, ids, weights, offsets, mode)), mode
        empty = int(np.flatnonzero(np.diff(offsets) == 0)[0])
        assert np.all(got[empty].view(np.uint32) == 0) and np.all(got[-2].view(np.uint32) == 0)     # empty / padding: +0.0


def test_the_definition_is_not_vacuous():
    """in numpy alone: float32 rounding happens, the order matters, and the segments matter"""
    rng = np.random.default_rng(17)
    dim = 200
    for bitlevel in (1, 2):
        _, table = make_table(rng, ROWS, dim, bitlevel)
        codes = codes_of(table, bitlevel)
        ids = rng.integers(0, ROWS, 2500).astype(np.int32)
        weights = dyadic_weights(rng, 2500)
        off = np.array([0, 2500], np.int64)
        one = chain(codes, ids[:1000], weights[:1000])
        exact = (weights[:1000].astype(np.float64)[:, None] * codes[ids[:1000]]).sum(axis=0)      # exact: multiples of 2^-6 < 2^36
        assert (one.astype(np.float64) != exact).any()                                            # (a)
        perm = rng.permutation(1000)
        assert (chain(codes, ids[:1000][perm], weights[:1000][perm]).view(np.uint32) != one.view(np.uint32)).any()   # (b)
        seg = ref_weighted(codes, bitlevel, ids, weights, off, "sum")
        flat = ref_weighted(codes, bitlevel, ids, weights, off, "sum", seg=1 << 30)
        assert (seg.view(np.uint32) != flat.view(np.uint32)).any()                                # (c)


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_unit_weights_equal_the_unweighted_twin_and_powers_of_two_scale_exactly(bitlevel):
    rng = np.random.default_rng(40 + bitlevel)
    dim = 65
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    ids, offsets = make_bags(rng, ROWS, extra=[70_000])
    ones = np.ones(len(ids), np.float32)
    for code in (0, 1):
        rc, want = host_bag(packed, dim, bitlevel, ids, offsets, code)
        rc2, got = host_bag_weighted(packed, dim, bitlevel, ids, ones, offsets, code)
        assert rc == 0 and rc2 == 0 and same_bits(got, want), code
    ids, offsets = make_bags(rng, ROWS)
    weights = dyadic_weights(rng, len(ids), kmax=(1 << 16) - 1)            # 2^-6 .. 2^10: in range after both scalings
    for code in (0, 1):
        rc, base = host_bag_weighted(packed, dim, bitlevel, ids, weights, offsets, code)
        assert rc == 0 and np.abs(base).max() > 1.0
        for s in (50, -40):
            rc, got = host_bag_weighted(packed, dim, bitlevel, ids, np.ldexp(weights, s).astype(np.float32), offsets, code)
            assert rc == 0 and same_bits(got, np.ldexp(base, s).astype(np.float32)), (code, s)


def test_validation_of_weights():
    rng = np.random.default_rng(6)
    dim = 65
    packed, _ = make_table(rng, ROWS, dim, 2)
    err = lambda: _lib.lib().w2b_last_error().decode()
    ids = np.array([1, 2, -1, 3, 7], np.int32)
    off = np.array([0, 2, 5], np.int64)
    good = np.array([1.0, -0.5, 3.0, 0.0, 2.0 ** 60], np.float32)
    rc, out = host_bag_weighted(packed, dim, 2, ids, good, off, 0)
    assert rc == 0 and not np.isnan(out).any()
    rc, out = host_bag_weighted(packed, dim, 2, ids, np.array([2.0 ** -60, -2.0 ** 60, 0, -0.0, 1], np.float32), off, 1)
    assert rc == 0                                                          # the ends of the range and both zeros
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** -61, 2.0 ** 61, -2.0 ** 61, 1e-45):
        w = good.copy()
        w[3] = bad
        rc, out = host_bag_weighted(packed, dim, 2, ids, w, off, 0)
        assert rc == _lib.W2B_EINVAL and "weights[3]" in err() and np.isnan(out).all(), bad       # nothing written
        w = good.copy()
        w[2] = bad                                                          # on a padding id: ignored
        rc, out2 = host_bag_weighted(packed, dim, 2, ids, w, off, 0)
        rc0, out0 = host_bag_weighted(packed, dim, 2, ids, good, off, 0)
        assert rc == 0 and rc0 == 0 and same_bits(out2, out0), bad
    rc, out = host_bag_weighted(packed, dim, 2, ids, good, off, 0, null_weights=True)
    assert rc == _lib.W2B_EINVAL and "weights" in err() and np.isnan(out).all()
    rc, _ = host_bag_weighted(packed, dim, 2, ids, good, off, 2)
    assert rc == _lib.W2B_EINVAL and "mode" in err()
    rc, _ = host_bag_weighted(packed, dim, 2, ids, good, np.array([0, 3, 2, 5], np.int64), 0)
    assert rc == _lib.W2B_EINVAL and "decrease" in err()
    rc, _ = host_bag_weighted(packed, dim, 2, ids, good, np.array([1, 2, 5], np.int64), 0)
    assert rc == _lib.W2B_EINVAL and "offsets[0]" in err()
    rc, _ = host_bag_weighted(packed, dim, 2, ids, good, np.array([0, 2, 4], np.int64), 0)
    assert rc == _lib.W2B_EINVAL and "offsets[n_bags]" in err()
    rc, out = host_bag_weighted(packed, dim, 2, np.array([1, ROWS, 2, 3, 4], np.int32), good, off, 0)
    assert rc == _lib.W2B_EINVAL and "rows" in err() and np.isnan(out).all()
    rc, _ = host_bag_weighted(packed, dim, 3, ids, good, off, 0)
    assert rc == _lib.W2B_EUNSUPPORTED
    rc, _ = host_bag_weighted(packed, dim, 2, np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(1, np.int64), 0)
    assert rc == 0                                                          # n_bags == 0
