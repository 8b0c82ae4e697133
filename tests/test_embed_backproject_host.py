"""The packed embedding's back-projection (include/word2bits_embed.h, "Back-projection"), the part that needs no GPU: the
ABI, the host twin against the numpy definition of the weighted bag (tests/test_embed_weighted_host.py: one bag per vector,
mode sum) and against the weighted bag's own twin, the consequences the header states, and every refusal with its cause.
No tolerance anywhere: every comparison is on bit patterns."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT
from test_embed_host import host_lookup, make_table, same_bits
from test_embed_project_host import host_project, wide_values
from test_embed_weighted_host import WSEG, codes_of, dyadic_weights, host_bag_weighted, ref_weighted

SYMBOLS = ("w2b_embed_backproject", "w2b_embed_reserve_backproject", "w2b_embed_backproject_device",
           "w2b_embed_backproject_host")
ROWS = 300
MS = [1, 2, 1023, 1024, 1025, 2500]


def host_backproject(packed, dim, bitlevel, g, cand, n=None, m=None, rows=None):
    """w2b_embed_backproject_host: (rc, dx float32 [n, dim], filled with NaN before the call)"""
    g = None if g is None else np.ascontiguousarray(g, np.float32)
    cand = None if cand is None else np.ascontiguousarray(cand, np.int32)
    m = (packed.shape[0] if cand is None else cand.size) if m is None else m
    n = (0 if g is None else g.size // max(m, 1)) if n is None else n
    dx = np.full((max(n, 0), dim), np.nan, np.float32)
    # (an empty list is still a list: numpy's pointer to no elements is not NULL)
    rc = _lib.lib().w2b_embed_backproject_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0] if rows is None else rows, dim,
                                               bitlevel, n, None if g is None else g.ctypes.data_as(_lib.f32p), m,
                                               None if cand is None else cand.ctypes.data_as(_lib.i32p),
                                               dx.ctypes.data_as(_lib.f32p))
    return rc, dx


def cand_list(rng, rows, m):
    """m candidates with repeats; padding at the first, a middle and the last position where m allows (m = 9 or >= 14)"""
    cand = rng.integers(0, rows, m).astype(np.int32)
    if m >= 9:
        cand[[5, 6, m - 2]] = cand[2], cand[2], rows - 1
        cand[[0, m // 2, m - 1]] = -1, -3, -1
    return cand


def as_bags(cand, g):
    """the weighted-bag call of consequence (a): ids = cand once per vector, weights = g, one bag per vector"""
    n, m = g.shape
    return np.tile(cand, n).astype(np.int32), np.ascontiguousarray(g).reshape(-1), np.arange(n + 1, dtype=np.int64) * m


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_embed.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int, name
        assert re.search(r"^int\s*%s\(" % name, header, flags=re.M), name
    for method in ("backproject", "reserve_backproject", "backproject_device", "staging_backproject", "torch_backproject"):
        assert callable(getattr(w2b.PackedEmbedding, method, None)), method
    assert "Gradients or training through the lookup (the table is read-only)" in header
    scope = header[header.index("---- out of scope"):header.index("#ifndef WORD2BITS_EMBED_H")]
    assert "with respect to x" not in scope and "with respect to the table" in scope and "second derivatives" in scope


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 3, 64, 65, 200])
def test_twin_equals_the_definition_of_the_weighted_bag(dim, bitlevel):
    """dyadic g (k / 64: the float64 step of ref_weighted's chain is then the fused multiply-add exactly) against the numpy
    definition and the weighted bag's twin; g over the whole allowed range, where numpy's step would round twice, against
    the weighted bag's twin, which that file ties to the definition"""
    rng = np.random.default_rng(1000 * dim + bitlevel)
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    codes = codes_of(table, bitlevel)
    n = 3
    for m in MS:
        cand = cand_list(rng, ROWS, m)
        g = dyadic_weights(rng, n * m).reshape(n, m)
        g[:, ::97] = 0.0
        ids, weights, offsets = as_bags(cand, g)
        rc, got = host_backproject(packed, dim, bitlevel, g, cand)
        assert rc == 0 and same_bits(got, ref_weighted(codes, bitlevel, ids, weights, offsets, "sum")), m
        rc, bag = host_bag_weighted(packed, dim, bitlevel, ids, weights, offsets, 0)
        assert rc == 0 and same_bits(got, bag), m
        gw = wide_values(rng, (n, m))
        gw[:, cand < 0] = np.nan                                               # g on padding is not looked at
        ids, weights, offsets = as_bags(cand, np.where(np.isnan(gw), np.float32(1.0), gw))
        rc, got = host_backproject(packed, dim, bitlevel, gw, cand)
        rc2, bag = host_bag_weighted(packed, dim, bitlevel, ids, weights, offsets, 0)
        assert rc == 0 and rc2 == 0 and same_bits(got, bag), m
    # every row in row order
    g = wide_values(rng, (n, ROWS))
    rc, got = host_backproject(packed, dim, bitlevel, g, None)
    rc2, listed = host_backproject(packed, dim, bitlevel, g, np.arange(ROWS, dtype=np.int32))
    ids, weights, offsets = as_bags(np.arange(ROWS), g)
    rc3, bag = host_bag_weighted(packed, dim, bitlevel, ids, weights, offsets, 0)
    assert rc == 0 and rc2 == 0 and rc3 == 0 and same_bits(got, listed) and same_bits(got, bag)


def test_the_segments_matter_for_the_inputs_used():
    """in numpy alone: at m = 2500 the segmented sum differs from the single chain over all positions, for the dyadic g
    (where numpy's chain is the definition) and for the wide-range g (where it is the definition up to a second rounding
    per step: still two different sums); so a twin that passes with a wrong segmentation is not possible above"""
    rng = np.random.default_rng(17)
    dim = 200
    for bitlevel in (1, 2):
        _, table = make_table(rng, ROWS, dim, bitlevel)
        codes = codes_of(table, bitlevel)
        cand = cand_list(rng, ROWS, 2500)
        for g in (dyadic_weights(rng, 2500), wide_values(rng, (2500,))):
            off = np.array([0, 2500], np.int64)
            seg = ref_weighted(codes, bitlevel, cand, g, off, "sum")
            flat = ref_weighted(codes, bitlevel, cand, g, off, "sum", seg=1 << 30)
            assert (seg.view(np.uint32) != flat.view(np.uint32)).any()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 65, 200])
def test_one_hot_reads_the_table(dim, bitlevel):
    rng = np.random.default_rng(77 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    cand = cand_list(rng, ROWS, 1100)                                          # unit positions in both segments
    rc, got = host_backproject(packed, dim, bitlevel, np.eye(1100, dtype=np.float32), cand)
    rc2, rows = host_lookup(packed, dim, bitlevel, cand)
    assert rc == 0 and rc2 == 0 and same_bits(got, rows)                       # a padding position reads +0.0
    rc, got = host_backproject(packed, dim, bitlevel, np.eye(ROWS, dtype=np.float32), None)
    rc2, rows = host_lookup(packed, dim, bitlevel, np.arange(ROWS, dtype=np.int32))
    assert rc == 0 and rc2 == 0 and same_bits(got, rows)


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("shift", [20, -20])
def test_scaling_by_a_power_of_two_is_exact(bitlevel, shift):
    rng = np.random.default_rng(41 + bitlevel)
    dim, m = 200, 2500
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    g = wide_values(rng, (4, m))
    g = np.where(np.abs(g) > 2.0 ** 39, g * np.float32(2.0 ** -21), g)         # stay in range after the shift
    g = np.where((g != 0) & (np.abs(g) < 2.0 ** -39), g * np.float32(2.0 ** 21), g).astype(np.float32)
    cand = cand_list(rng, ROWS, m)
    rc, base = host_backproject(packed, dim, bitlevel, g, cand)
    rc2, scaled = host_backproject(packed, dim, bitlevel, g * np.float32(2.0 ** shift), cand)
    assert rc == 0 and rc2 == 0 and np.abs(base).max() > 0 and same_bits(scaled, base * np.float32(2.0 ** shift))


def test_it_is_the_adjoint_of_the_projection():
    """bitlevel 2 (q = 1 / 4 exactly), x and g integers in [-8, 8], dim 200, m = 300: every sum is an integer below 2^24,
    so both twins are exact and 4 * out, 4 * dx are integers; <g, project(x)> == <x, backproject(g)> in Python integers"""
    rng = np.random.default_rng(53)
    dim, m, n = 200, 300, 5
    packed, _ = make_table(rng, ROWS, dim, 2)
    cand = cand_list(rng, ROWS, m)
    x = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    g = rng.integers(-8, 9, (n, m)).astype(np.float32)
    rc, y = host_project(packed, dim, 2, x, cand)
    rc2, dx = host_backproject(packed, dim, 2, g, cand)
    assert rc == 0 and rc2 == 0
    y4, dx4 = y.astype(np.float64) * 4, dx.astype(np.float64) * 4
    assert np.array_equal(y4, np.rint(y4)) and np.array_equal(dx4, np.rint(dx4))
    lhs = sum(int(a) * int(b) for a, b in zip(g.ravel(), y4.ravel()))
    rhs = sum(int(a) * int(b) for a, b in zip(x.ravel(), dx4.ravel()))
    assert lhs == rhs and lhs != 0


def test_every_refusal_names_its_cause_and_leaves_dx_untouched():
    rng = np.random.default_rng(6)
    dim, bitlevel = 65, 2
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    L = _lib.lib()
    err = lambda: L.w2b_last_error().decode()
    cand = cand_list(rng, ROWS, 9)                                            # padding at 0, 4 and 8
    g = wide_values(rng, (4, 9))

    def refused(rc, dx, *words):
        assert rc == _lib.W2B_EINVAL and all(w in err() for w in words), (rc, err())
        assert np.isnan(dx).all()

    rc0, base = host_backproject(packed, dim, bitlevel, g, cand)
    assert rc0 == 0 and not np.isnan(base).any()
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 61, -(2.0 ** -61), 1e-45):
        y = g.copy()
        y[2, 7] = bad
        refused(*host_backproject(packed, dim, bitlevel, y, cand), "vector 2", "candidate 7")
        y = g.copy()
        y[2, 4] = bad                                                         # on a padding candidate: accepted, ignored
        rc, dx = host_backproject(packed, dim, bitlevel, y, cand)
        assert rc == 0 and same_bits(dx, base), bad
    full = wide_values(rng, (2, ROWS))
    full[1, 17] = np.nan
    refused(*host_backproject(packed, dim, bitlevel, full, None), "vector 1", "candidate 17")
    y = g.copy()
    y[0, 1], y[3, 7], y[1, 2] = 2.0 ** 60, -(2.0 ** -60), -0.0                # the bounds themselves are fine
    rc, dx = host_backproject(packed, dim, bitlevel, y, cand)
    assert rc == 0 and not np.isnan(dx).any()
    c = cand.copy()
    c[5] = ROWS
    refused(*host_backproject(packed, dim, bitlevel, g, c), "cand[5]", "rows")
    y = g.copy()
    y[0, 1] = np.nan                                                          # candidates come before values
    refused(*host_backproject(packed, dim, bitlevel, y, c), "cand[5]")
    refused(*host_backproject(packed, dim, bitlevel, full, None, n=2, m=ROWS - 1), "must be rows")
    refused(*host_backproject(packed, dim, bitlevel, g, cand, n=-1), "vector count")
    refused(*host_backproject(packed, dim, bitlevel, g, cand, m=-1), "candidate count")
    refused(*host_backproject(packed, dim, bitlevel, None, cand, n=4), "null g")
    a = (packed.ctypes.data_as(_lib.u64p), ROWS, dim, bitlevel, 4, g.ctypes.data_as(_lib.f32p), 9, cand.ctypes.data_as(_lib.i32p))
    assert L.w2b_embed_backproject_host(*a, None) == _lib.W2B_EINVAL and "null output" in err()
    dx = np.full((4, dim), np.nan, np.float32)
    dxp = dx.ctypes.data_as(_lib.f32p)
    assert L.w2b_embed_backproject_host(None, *a[1:], dxp) == _lib.W2B_EINVAL and "null table" in err()
    assert L.w2b_embed_backproject_host(a[0], ROWS, dim, 3, *a[4:], dxp) == _lib.W2B_EUNSUPPORTED
    assert np.isnan(dx).all()
    # n == 0 is fine, with or without pointers; m == 0 gives +0.0 rows
    assert host_backproject(packed, dim, bitlevel, None, cand, n=0)[0] == 0
    assert L.w2b_embed_backproject_host(*a[:4], 0, None, 9, a[7], None) == 0
    rc = L.w2b_embed_backproject_host(*a[:4], 4, None, 0, cand.ctypes.data_as(_lib.i32p), dxp)
    assert rc == 0 and np.all(dx.view(np.uint32) == 0)

    # the host form: what needs no handle comes first, so it is refused without a device and without a handle
    dx[:] = np.nan

    def form(n, gp, m, cp, outp, h=None):
        return L.w2b_embed_backproject(h, n, gp, m, cp, outp)
    gp, cp = a[5], a[7]
    assert form(-1, gp, 9, cp, dxp) == _lib.W2B_EINVAL and "vector count" in err()
    assert form((1 << 24) + 1, gp, 9, cp, dxp) == _lib.W2B_EINVAL and "vector count" in err()
    assert form(4, gp, -2, cp, dxp) == _lib.W2B_EINVAL and "candidate count" in err()
    assert form(4, gp, 0x7FFFFF01, cp, dxp) == _lib.W2B_EINVAL and "candidate count" in err()
    assert form(4, None, 9, cp, dxp) == _lib.W2B_EINVAL and "null g" in err()
    assert form(4, gp, 9, cp, None) == _lib.W2B_EINVAL and "null output" in err()
    assert form(4, gp, 9, cp, dxp) == _lib.W2B_EINVAL and "null handle" in err()
    assert form(0, None, 0, None, None) == _lib.W2B_EINVAL and "null handle" in err()
    assert L.w2b_embed_reserve_backproject(None, 1, 1, None, None, None) == _lib.W2B_EINVAL
    assert L.w2b_embed_backproject_device(None, 1, 1, 1) == _lib.W2B_EINVAL
    assert np.isnan(dx).all()
