"""The packed embedding's projection (include/word2bits_embed.h, "Projection"), the part that needs no GPU: the ABI, the
host twin against a numpy definition (the float64 restatement of one fmaf per column that tests/vectors_testlib.py uses
for the vector questions; bit for bit), the three consequences the header states, and every refusal with its cause."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT
from test_embed_host import Q1, host_lookup, make_table
from vectors_testlib import host_vector, numpy_vector

SYMBOLS = {"w2b_embed_project": "int", "w2b_embed_reserve_project": "int", "w2b_embed_project_device": "int",
           "w2b_embed_project_host": "int"}
ROWS = 300


def q_of(bitlevel):
    return Q1 if bitlevel == 1 else np.float32(0.25)


def codes_of(table, bitlevel):
    """the integer matrix t [rows, dim] of an unpacked table: +-1, or +-1 / +-3"""
    codes = np.rint(table.astype(np.float64) / np.float64(q_of(bitlevel))).astype(np.int64)
    assert set(np.unique(codes).tolist()) <= ({-1, 1} if bitlevel == 1 else {-3, -1, 1, 3})
    return codes


def wide_values(rng, shape):
    """the whole allowed range, as wide_weights of tests/test_gpu_embed_weighted.py draws it: random sign, exponent
    -60 .. 59, random mantissa, and some zeros of either sign"""
    n = int(np.prod(shape))
    bits = (rng.integers(0, 2, n).astype(np.uint32) << 31) | ((127 + rng.integers(-60, 60, n)).astype(np.uint32) << 23) | \
        rng.integers(0, 1 << 23, n).astype(np.uint32)
    bits[rng.random(n) < 0.03] &= np.uint32(0x80000000)
    return bits.view(np.float32).reshape(shape)


def host_project(packed, dim, bitlevel, x, cand, n=None, m=None, rows=None):
    """w2b_embed_project_host: (rc, out float32 [n, m], filled with NaN before the call)"""
    x = None if x is None else np.ascontiguousarray(x, np.float32)
    cand = None if cand is None else np.ascontiguousarray(cand, np.int32)
    n = (0 if x is None else x.size // dim) if n is None else n
    m = (packed.shape[0] if cand is None else cand.size) if m is None else m
    out = np.full((max(n, 0), max(m, 0)), np.nan, np.float32)
    rc = _lib.lib().w2b_embed_project_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0] if rows is None else rows, dim,
                                           bitlevel, n, None if x is None else x.ctypes.data_as(_lib.f32p), m,
                                           None if cand is None else cand.ctypes.data_as(_lib.i32p),
                                           out.ctypes.data_as(_lib.f32p))
    return rc, out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def candidates(rng, rows, m):
    """m candidates with repeats and padding (where m allows), the first and the last row among them"""
    cand = rng.integers(0, rows, m).astype(np.int32)
    if m >= 8:
        cand[[1, m - 2]] = -1, -5
        cand[3] = cand[0]
        cand[[2, m - 1]] = 0, rows - 1
    return cand


def numpy_project(codes, bitlevel, x, cand):
    """the definition: numpy_vector's chain (float64 sums of a float32 accumulator and an exact product: one rounding per
    column) for every vector, all rows at once; then the one float32 multiply; padding candidates are +0.0"""
    S = np.stack([numpy_vector(codes, bitlevel, xi, 0)[0] for xi in x])          # [n, rows]
    assert S.dtype == np.float32
    full = S * q_of(bitlevel)
    assert full.dtype == np.float32
    if cand is None:
        return full
    out = full[:, np.maximum(cand, 0)].copy()
    out[:, cand < 0] = 0.0
    return out


def round_f32(v):
    """the exact rational v rounded ONCE to float32, ties to even (through float64 it would be rounded twice: the float64
    neighbour is at most one float32 step off, so the nearest of three is taken exactly)"""
    f = np.float32(float(v))
    near = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    dist = [abs(Fraction(float(c)) - v) for c in near]
    best = min(dist)
    tied = [c for c, d in zip(near, dist) if d == best]
    if len(tied) > 1:
        tied = [c for c in tied if not (int(c.view(np.uint32)) & 1)]
    return np.float32(tied[0]) + np.float32(0.0)                                           # an exact zero is +0.0


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_embed.h")).read()
    for name, res in SYMBOLS.items():
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int, name
        assert re.search(r"^%s\s*%s\(" % (res, name), header, flags=re.M), name
    for method in ("project", "reserve_project", "project_device", "staging_project", "torch_project"):
        assert callable(getattr(w2b.PackedEmbedding, method, None)), method
    assert "Gradients or training through the lookup" in header


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 3, 64, 65, 200, 513])
def test_twin_equals_the_numpy_definition(dim, bitlevel):
    """numpy_vector's float64 step is the correctly rounded fmaf when acc + x * t is exact in float64.  Over the whole
    exponent range that does not hold in general, so the wide-range values are compared through Python's exact rational
    arithmetic on a few entries, and the bulk with exponents close together (53 bits hold every sum exactly)."""
    rng = np.random.default_rng(1000 * dim + bitlevel)
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    codes = codes_of(table, bitlevel)
    cand = candidates(rng, ROWS, 40)
    # (a) exponents within 2^-10 .. 2^10 around a common scale: acc and x * t differ by fewer than 53 - 24 - 2 bits
    x = (wide_values(rng, (7, dim)).astype(np.float64))
    mant, _ = np.frexp(x)
    x = (np.ldexp(mant, rng.integers(-10, 11, x.shape)) * 2.0 ** 40).astype(np.float32)
    for c in (None, cand):
        rc, got = host_project(packed, dim, bitlevel, x, c)
        assert rc == 0 and same_bits(got, numpy_project(codes, bitlevel, x, c))
    assert not np.signbit(got[:, cand < 0]).any() and not got[:, cand < 0].any()         # padding columns are +0.0
    assert same_bits(got[:, 3], got[:, 0])                                                 # a repeated row repeats
    # (b) the whole allowed range, zeros of either sign included: exact rationals, rounded once per column
    xw = wide_values(rng, (3, dim))
    xw[0, 0] = np.float32(-0.0)
    assert (xw == 0).any() or dim < 40
    rc, got = host_project(packed, dim, bitlevel, xw, cand)
    assert rc == 0
    for i in range(3):
        for j in (0, 1, 2, 5, 20, 39):
            S = np.float32(0)
            if cand[j] >= 0:
                for a in range(dim):
                    S = round_f32(Fraction(float(xw[i, a])) * int(codes[cand[j], a]) + Fraction(float(S)))
            want = S * q_of(bitlevel)
            assert got[i, j].view(np.uint32) == np.float32(want).view(np.uint32), (i, j)


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 65, 200])
def test_unit_vectors_read_the_table(dim, bitlevel):
    rng = np.random.default_rng(77 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    cand = candidates(rng, ROWS, 33)
    rc, got = host_project(packed, dim, bitlevel, np.eye(dim, dtype=np.float32), cand)
    rc2, rows = host_lookup(packed, dim, bitlevel, cand)
    assert rc == 0 and rc2 == 0 and same_bits(got, np.ascontiguousarray(rows.T))
    rc, got = host_project(packed, dim, bitlevel, np.eye(dim, dtype=np.float32), None)
    rc2, rows = host_lookup(packed, dim, bitlevel, np.arange(ROWS, dtype=np.int32))
    assert rc == 0 and rc2 == 0 and same_bits(got, np.ascontiguousarray(rows.T))


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_the_chain_is_that_of_the_vector_questions(bitlevel):
    """S_out of w2b_vector_scores_host, times q in numpy, is the twin's output (out / q is not S in general)"""
    rng = np.random.default_rng(31 + bitlevel)
    dim = 130
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    x = wide_values(rng, (4, dim))
    rc, got = host_project(packed, dim, bitlevel, x, None)
    assert rc == 0
    for i in range(4):
        rc, S, _ = host_vector(packed, dim, bitlevel, x[i], 0)
        assert rc == 0 and S.dtype == np.float32
        assert same_bits(got[i], S * q_of(bitlevel)), i


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("shift", [20, -20])
def test_scaling_by_a_power_of_two_is_exact(bitlevel, shift):
    rng = np.random.default_rng(41 + bitlevel)
    dim = 200
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    x = wide_values(rng, (5, dim))
    x = np.where(np.abs(x) > 2.0 ** 39, x * np.float32(2.0 ** -21), x)                    # stay in range after the shift
    x = np.where((x != 0) & (np.abs(x) < 2.0 ** -39), x * np.float32(2.0 ** 21), x).astype(np.float32)
    cand = candidates(rng, ROWS, 50)
    rc, base = host_project(packed, dim, bitlevel, x, cand)
    rc2, scaled = host_project(packed, dim, bitlevel, x * np.float32(2.0 ** shift), cand)
    assert rc == 0 and rc2 == 0 and same_bits(scaled, base * np.float32(2.0 ** shift))


def test_every_refusal_names_its_cause_and_leaves_out_untouched():
    rng = np.random.default_rng(6)
    dim, bitlevel = 65, 2
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    L = _lib.lib()
    err = lambda: L.w2b_last_error().decode()
    x = wide_values(rng, (4, dim))
    cand = candidates(rng, ROWS, 9)

    def refused(rc, out, *words):
        assert rc == _lib.W2B_EINVAL and all(w in err() for w in words), (rc, err())
        assert np.isnan(out).all()

    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 61, -(2.0 ** -61), 1e-45):
        y = x.copy()
        y[2, 17] = bad
        refused(*host_project(packed, dim, bitlevel, y, cand), "vector 2", "column 17")
        refused(*host_project(packed, dim, bitlevel, y, None), "vector 2", "column 17")
    y = x.copy()
    y[0, 0], y[3, 64], y[1, 1] = 2.0 ** 60, -(2.0 ** -60), -0.0                           # the bounds themselves are fine
    rc, out = host_project(packed, dim, bitlevel, y, cand)
    assert rc == 0 and not np.isnan(out).any()
    c = cand.copy()
    c[5] = ROWS
    refused(*host_project(packed, dim, bitlevel, x, c), "cand[5]", "rows")
    y = x.copy()
    y[0, 0] = np.nan                                                                      # candidates come before values
    refused(*host_project(packed, dim, bitlevel, y, c), "cand[5]")
    refused(*host_project(packed, dim, bitlevel, x, None, m=ROWS - 1), "must be rows")
    refused(*host_project(packed, dim, bitlevel, x, cand, n=-1), "vector count")
    refused(*host_project(packed, dim, bitlevel, x, cand, m=-1), "candidate count")
    refused(*host_project(packed, dim, bitlevel, None, cand, n=4), "null vectors")
    a = (packed.ctypes.data_as(_lib.u64p), ROWS, dim, bitlevel, 4, x.ctypes.data_as(_lib.f32p), 9, cand.ctypes.data_as(_lib.i32p))
    assert L.w2b_embed_project_host(*a, None) == _lib.W2B_EINVAL and "null output" in err()
    out = np.full((4, 9), np.nan, np.float32)
    assert L.w2b_embed_project_host(None, *a[1:], out.ctypes.data_as(_lib.f32p)) == _lib.W2B_EINVAL and "null table" in err()
    assert L.w2b_embed_project_host(a[0], ROWS, dim, 3, *a[4:], out.ctypes.data_as(_lib.f32p)) == _lib.W2B_EUNSUPPORTED
    assert np.isnan(out).all()
    # n == 0 and m == 0 are fine, with or without pointers
    assert host_project(packed, dim, bitlevel, None, cand, n=0)[0] == 0
    assert host_project(packed, dim, bitlevel, x, np.zeros(0, np.int32))[0] == 0
    assert L.w2b_embed_project_host(*a[:6], 0, a[7], None) == 0
    assert L.w2b_embed_project_host(*a[:6], 0, None, None) == _lib.W2B_EINVAL and "must be rows" in err()    # NULL = every row

    # the host form: what needs no handle comes first, so it is refused without a device and without a handle
    def form(n, xp, m, cp, dtype, outp, h=None):
        return L.w2b_embed_project(h, n, xp, m, cp, dtype, outp)
    xp, cp, op = a[5], a[7], C.c_void_p(out.ctypes.data)
    assert form(4, xp, 9, cp, 7, op) == _lib.W2B_EINVAL and "dtype" in err()
    assert form(-1, xp, 9, cp, 0, op) == _lib.W2B_EINVAL and "vector count" in err()
    assert form(4, xp, -2, cp, 0, op) == _lib.W2B_EINVAL and "candidate count" in err()
    assert form(4, None, 9, cp, 0, op) == _lib.W2B_EINVAL and "null vectors" in err()
    assert form(4, xp, 9, cp, 0, None) == _lib.W2B_EINVAL and "null output" in err()
    assert form(4, xp, 9, cp, 0, op) == _lib.W2B_EINVAL and "null handle" in err()
    assert form(0, None, 0, None, 0, None) == _lib.W2B_EINVAL and "null handle" in err()
    assert L.w2b_embed_reserve_project(None, 1, 1, 0, None, None, None) == _lib.W2B_EINVAL
    assert L.w2b_embed_project_device(None, 1, 1, 1, 0) == _lib.W2B_EINVAL
    assert np.isnan(out).all()
