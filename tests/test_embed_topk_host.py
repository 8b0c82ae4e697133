"""The packed embedding's top-k selection (include/word2bits_embed.h, "Top-k"), the part that needs no GPU: the ABI, the host
twin against w2b_embed_project_host followed by a stable sort in numpy (bit for bit), the consequences the header states,
every refusal in its stated order with the outputs untouched, and the stand-alone sanitizer program of the twin.  The inputs
of tests/test_gpu_embed_topk.py are made here (case()), with the proof that every kind of input reaches the branch it is
meant for."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT
from test_embed_host import make_table
from test_embed_project_host import host_project, same_bits
from test_embed_xent_host import host_xent

SYMBOLS = ("w2b_embed_topk", "w2b_embed_reserve_topk", "w2b_embed_topk_device", "w2b_embed_topk_host")
ROWS = 300
TWINS = 64                   # rows 0 .. 63 of a table of make_case are near-duplicates of row 0
MAX_K = 64
MS = [1, 2, 255, 256, 257, 1025, 2500]
KS = [1, 2, 31, 32, 33, 64]
NEG_INF = np.float32(-np.inf)


def host_topk(packed, dim, bitlevel, x, cand, k, n=None, m=None, rows=None, vals=True, pos=True):
    """w2b_embed_topk_host: (rc, vals float32 [n, k], pos int32 [n, k]); vals is NaN and pos -77 before the call"""
    x = None if x is None else np.ascontiguousarray(x, np.float32)
    cand = None if cand is None else np.ascontiguousarray(cand, np.int32)
    n = (0 if x is None else x.size // dim) if n is None else n
    m = (packed.shape[0] if cand is None else cand.size) if m is None else m
    kk = min(max(k, 1), 2 * MAX_K)
    v, p = np.full((max(n, 0), kk), np.nan, np.float32), np.full((max(n, 0), kk), -77, np.int32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    rc = _lib.lib().w2b_embed_topk_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0] if rows is None else rows, dim, bitlevel,
                                        n, ptr(x, _lib.f32p), m, ptr(cand, _lib.i32p), k, ptr(v, _lib.f32p) if vals else None,
                                        ptr(p, _lib.i32p) if pos else None)
    return rc, v, p


def numpy_topk(l, cand, k):
    """the header's consequence (a) for the logits l [n, m] of the projection's twin: per vector the live positions in a
    stable descending sort -- np.lexsort on (position, -value) --, the first k of them, then pos = -1, val = -inf"""
    n, m = l.shape
    live = np.arange(m) if cand is None else np.flatnonzero(cand >= 0)
    vals, pos = np.full((n, k), NEG_INF, np.float32), np.full((n, k), -1, np.int32)
    for i in range(n):
        order = live[np.lexsort((live, -l[i, live]))][:k]
        vals[i, :len(order)] = l[i, order]
        pos[i, :len(order)] = order
    return vals, pos


def twin(packed, dim, bitlevel, x, cand, k=MAX_K):
    rc, vals, pos = host_topk(packed, dim, bitlevel, x, cand, k)
    assert rc == 0, _lib.lib().w2b_last_error()
    return vals, pos


def topk_table(rng, rows, dim, bitlevel):
    """a random table whose rows 1 .. TWINS - 1 are row 0 with at most dim // 8 signs flipped (and, at two bits, magnitudes
    of their own): against x = -c sign(row 0) every one of them has a negative logit, at least -(7/8 - 3/8) c dim / 4"""
    packed, table = make_table(rng, rows, dim, bitlevel)
    vals = table.copy()
    for r in range(1, TWINS):
        mags = np.abs(vals[r])
        flip = np.ones(dim, np.float32)
        flip[rng.permutation(dim)[:rng.integers(0, dim // 8 + 1)]] = -1
        vals[r] = np.sign(vals[0]) * flip * mags
    packed = w2b.pack_quantized(vals, bitlevel)
    return packed, w2b.unpack_quantized(packed, dim, bitlevel)


def topk_cands(rng, rows, m):
    """m candidates with repeats and, from m = 8 on, padding sprinkled in (about one in eight, the first and the last
    position among them) and one row standing three times"""
    cand = rng.integers(0, rows, m).astype(np.int32)
    if m >= 8:
        cand[rng.random(m) < 0.125] = -1
        cand[[0, m - 1]] = -1, -4
        cand[[2, 5, m - 2]] = cand[3]
    return cand


def x_gauss(rng, n, dim):
    return rng.standard_normal((n, dim)).astype(np.float32)


def x_ints(rng, n, dim):
    """small integers: on a one-bit table every logit is an integer in [-dim, dim] times q, so lists longer than that tie"""
    return rng.integers(-1, 2, (n, dim)).astype(np.float32)


def x_negative(rng, table, n):
    """-c sign(row 0), c a power of two per vector: every logit against the rows 0 .. TWINS - 1 is negative"""
    c = np.exp2(rng.integers(-3, 4, (n, 1))).astype(np.float32)
    return (-c * np.sign(table[0])[None, :]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(dim, bitlevel):
    """Per (dim, bitlevel) a table of 300 rows and a list of (name, cand, x, (vals, pos)) with the twin's answer for k = 64
    (a smaller k is a prefix of it, fewer vectors are its first rows): per m of MS and for all rows ("all", cand None) the
    sets "gauss" (130 vectors), "ints" (65) and "zero" (2); "sparse", 257 positions of which 5 are live, with gauss; "neg",
    1025 positions on the near-duplicates of row 0 with padding, with x_negative (33).  Then a table of 2100 rows with 130
    gauss vectors against all of it.  Everything is read-only."""
    rng = np.random.default_rng(23 * dim + bitlevel)
    packed, table = topk_table(rng, ROWS, dim, bitlevel)
    entries = []
    for m in MS + [None]:
        cand = None if m is None else topk_cands(rng, ROWS, m)
        for name, x in (("gauss", x_gauss(rng, 130, dim)), ("ints", x_ints(rng, 65, dim)), ("zero", np.zeros((2, dim), np.float32))):
            entries.append((name, cand, x))
    sparse = np.full(257, -1, np.int32)
    sparse[[3, 64, 65, 200, 256]] = rng.integers(0, ROWS, 5)
    entries.append(("sparse", sparse, x_gauss(rng, 65, dim)))
    near = rng.integers(0, TWINS, 1025).astype(np.int32)
    near[rng.random(1025) < 0.125] = -1
    entries.append(("neg", near, x_negative(rng, table, 33)))
    lists = [(name, cand, x, twin(packed, dim, bitlevel, x, cand)) for name, cand, x in entries]
    big, _ = make_table(rng, 2100, dim, bitlevel)
    xb = x_gauss(rng, 130, dim)
    wide = [("gauss", None, xb, twin(big, dim, bitlevel, xb, None))]
    for _, cand, x, want in lists + wide:
        for a in (cand, x, *want):
            if a is not None:
                a.setflags(write=False)
    return packed, table, lists, big, wide


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_embed.h")).read()
    mirror = open(os.path.join(ROOT, "include", "word2bits_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int, name
        assert re.search(r"^int\s*%s\(" % name, header, flags=re.M) and re.search(r"^int\s*%s\(" % name, mirror, flags=re.M), name
    for method in ("topk", "reserve_topk", "topk_device", "staging_topk", "torch_topk", "torch_sample"):
        assert callable(getattr(w2b.PackedEmbedding, method, None)), method
    assert re.search(r"#define\s+W2B_EMBED_MAX_K\s+64\b", header)
    assert "Top-k (w2b_embed_topk*" in header and "cannot be -0.0" in header


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 33, 65, 200])
def test_the_twin_is_the_projection_then_a_stable_sort(dim, bitlevel):
    """consequence (a), for every list and every set of case(), every k of KS; and a smaller k is a prefix of a larger one"""
    packed, table, lists, big, wide = case(dim, bitlevel)
    for tab, entries in ((packed, lists), (big, wide)):
        for name, cand, x, want in entries:
            x = x[:33]
            rc, l = host_project(tab, dim, bitlevel, x, cand)
            assert rc == 0
            for k in KS:
                rc, vals, pos = host_topk(tab, dim, bitlevel, x, cand, k)
                ref_v, ref_p = numpy_topk(l, cand, k)
                tag = (name, None if cand is None else len(cand), k)
                assert rc == 0 and same_bits(vals, ref_v) and np.array_equal(pos, ref_p), tag
                assert same_bits(vals, np.ascontiguousarray(want[0][:33, :k])) and np.array_equal(pos, want[1][:33, :k]), tag


def test_the_kinds_of_input_reach_the_branches_they_are_meant_for():
    """On the twin's results alone, at dim 200: the gaussian vectors against the 2100 random rows have no tie among their 64 best (so torch.topk
    is a witness for them); against the near-duplicates every answer is negative; the zero vector answers with the first k live
    positions at +0.0; the integer vectors on the one-bit table tie ACROSS the cut (the k-th and the (k + 1)-th logit are
    equal) for some vector at every k; "sparse" has fewer live positions than k; the lists of m >= 8 have padding, and a
    row that stands three times appears once per position, lowest first (consequence (c))."""
    for bitlevel in (1, 2):
        packed, table, lists, _, wide = case(200, bitlevel)
        assert (np.diff(wide[0][3][0], axis=1) < 0).all()              # (repeated and near-duplicate rows tie by construction)
        seen = set()
        for name, cand, x, (vals, pos) in lists:
            m = ROWS if cand is None else len(cand)
            live = np.arange(m) if cand is None else np.flatnonzero(cand >= 0)
            seen.add(name)
            if cand is not None and m >= 8 and name != "sparse":
                assert (cand < 0).any() and not np.isin(pos, np.flatnonzero(cand < 0)).any()
            if name == "neg":
                assert (pos >= 0).all() and (vals < 0).all() and (np.diff(vals.view(np.int32), axis=1) >= 0).all()
            if name == "zero":
                want = np.full(MAX_K, -1)
                want[:min(MAX_K, len(live))] = live[:MAX_K]
                assert (pos == want).all() and not vals[pos >= 0].view(np.uint32).any()
            if name == "sparse":
                assert len(live) == 5 and (pos[:, 5:] == -1).all() and (pos[:, :5] >= 0).all()
                assert (vals[:, 5:].view(np.uint32) == 0xFF800000).all()
            if name == "ints" and bitlevel == 1 and m >= 1025:
                rc, l = host_project(packed, 200, 1, x, cand)
                for k in KS:
                    rc, v1, p1 = host_topk(packed, 200, 1, x, cand, k + 1 if k < MAX_K else k)
                    kth = v1[:, k - 1]
                    nxt = v1[:, k] if k < MAX_K else np.array([np.sort(l[i, live])[::-1][k] for i in range(len(x))], np.float32)
                    assert (kth == nxt).any(), k
            if cand is not None and m >= 1025 and name == "zero":
                trio = [j for j in (2, 3, 5) if j in pos[0]]
                assert trio == [2, 3, 5] and cand[2] == cand[3] == cand[5]
                at = [int(np.flatnonzero(pos[0] == j)[0]) for j in trio]
                assert at == sorted(at)
        assert seen == {"gauss", "ints", "zero", "sparse", "neg"}


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_k_1_is_the_maximum_of_the_cross_entropy(bitlevel):
    """consequence (b): vals of k = 1 == mx of w2b_embed_xent_host for the same operands, wherever a position is live"""
    dim = 65
    packed, table, lists, _, _ = case(dim, bitlevel)
    for name, cand, x, want in lists:
        x = x[:33]
        rc, mx, se, tl, _ = host_xent(packed, dim, bitlevel, x, cand, np.full(len(x), -1, np.int32), grad=False)
        assert rc == 0
        rc, vals, pos = host_topk(packed, dim, bitlevel, x, cand, 1)
        assert rc == 0 and (pos >= 0).all() and same_bits(vals[:, 0], mx), name


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_scaling_x_by_a_power_of_two_scales_the_values_and_keeps_the_positions(bitlevel):
    """consequence (d), s >= 0"""
    dim = 200
    packed, table, lists, _, _ = case(dim, bitlevel)
    for name, cand, x, want in lists:
        if name not in ("gauss", "ints", "neg") or (cand is not None and len(cand) not in (257, 1025)):
            continue
        for s in (1, 7, 30):
            rc, vals, pos = host_topk(packed, dim, bitlevel, x[:9] * np.float32(2.0 ** s), cand, 33)
            assert rc == 0 and np.array_equal(pos, want[1][:9, :33]), (name, s)
            assert same_bits(vals, np.ascontiguousarray(want[0][:9, :33] * np.float32(2.0 ** s))), (name, s)


def test_empty_calls_and_lists_shorter_than_k():
    rng = np.random.default_rng(5)
    dim, bitlevel = 33, 2
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    x = x_gauss(rng, 4, dim)
    rc, vals, pos = host_topk(packed, dim, bitlevel, x, np.zeros(0, np.int32), 3)                   # m == 0: empty lists
    assert rc == 0 and (pos == -1).all() and (vals.view(np.uint32) == 0xFF800000).all()
    rc, vals, pos = host_topk(packed, dim, bitlevel, x, np.array([-1, -2, -1], np.int32), 2)         # nothing live
    assert rc == 0 and (pos == -1).all() and (vals.view(np.uint32) == 0xFF800000).all()
    rc, vals, pos = host_topk(packed, dim, bitlevel, None, np.array([1], np.int32), 2, vals=False, pos=False)   # n == 0
    assert rc == 0
    cand = np.array([7, -1, 7, 250], np.int32)
    rc, vals, pos = host_topk(packed, dim, bitlevel, x, cand, 64)                                   # k beyond the three live positions
    rc2, l = host_project(packed, dim, bitlevel, x, cand)
    ref_v, ref_p = numpy_topk(l, cand, 64)
    assert rc == 0 and rc2 == 0 and same_bits(vals, ref_v) and np.array_equal(pos, ref_p)
    assert (pos[:, 3:] == -1).all() and (np.sort(pos[:, :3], axis=1) == [0, 2, 3]).all()
    assert ((pos[:, :3] == 0).argmax(axis=1) < (pos[:, :3] == 2).argmax(axis=1)).all()               # the same row twice: lowest position first
    rc, vals, pos = host_topk(packed, dim, bitlevel, x, None, 64)                                    # all rows, k = 64 = the maximum
    assert rc == 0 and (pos >= 0).all() and all(len(set(r)) == 64 for r in pos.tolist())


def test_refusals_come_in_the_stated_order_and_leave_the_outputs_untouched():
    rng = np.random.default_rng(7)
    dim, bitlevel = 65, 1
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    x = x_gauss(rng, 3, dim)
    cand = np.array([5, -1, 299, 5], np.int32)
    err = lambda: _lib.lib().w2b_last_error().decode()

    def refused(code, cause, *args, **kw):
        rc, vals, pos = host_topk(packed, dim, bitlevel, *args, **kw)
        assert rc == code and cause in err(), (rc, err())
        assert np.isnan(vals).all() and (pos == -77).all()

    bad_cand, bad_x = cand.copy(), x.copy()
    bad_cand[2] = ROWS
    bad_x[1, 64] = np.inf
    # what needs no table: counts, then k, then NULL pointers
    refused(_lib.W2B_EINVAL, "bad vector count", x, cand, 0, n=-1, rows=-5)
    refused(_lib.W2B_EINVAL, "bad candidate count", x, cand, 0, m=-1, rows=-5)
    refused(_lib.W2B_EINVAL, "k = 0", None, bad_cand, 0, n=3, rows=-5)
    refused(_lib.W2B_EINVAL, "k = 65", None, bad_cand, 65, n=3, rows=-5)
    refused(_lib.W2B_EINVAL, "k = -1", None, bad_cand, -1, n=3, rows=-5)
    refused(_lib.W2B_EINVAL, "null vectors", None, bad_cand, 2, n=3, rows=-5)
    refused(_lib.W2B_EINVAL, "null output", bad_x, bad_cand, 2, rows=-5, vals=False)
    refused(_lib.W2B_EINVAL, "null output", bad_x, bad_cand, 2, rows=-5, pos=False)
    # then the table, then the candidates, then the values of x
    refused(_lib.W2B_EINVAL, "unsupported rows / dim", bad_x, bad_cand, 2, rows=-5)
    rc, vals, pos = host_topk(packed, dim, 3, bad_x, bad_cand, 2)
    assert rc == _lib.W2B_EUNSUPPORTED and np.isnan(vals).all() and (pos == -77).all()
    refused(_lib.W2B_EINVAL, "must be rows", bad_x, None, 2, m=5)
    refused(_lib.W2B_EINVAL, "cand[2] = 300", bad_x, bad_cand, 2)
    refused(_lib.W2B_EINVAL, "vector 1, column 64", bad_x, cand, 2)
    for v in (np.nan, -np.inf, 2.0 ** 61, 2.0 ** -61, 1e-45):
        bad_x[1, 64] = v
        refused(_lib.W2B_EINVAL, "vector 1, column 64", bad_x, cand, 2)
    rc, vals, pos = host_topk(packed, dim, bitlevel, x, cand, 2)
    assert rc == 0 and not np.isnan(vals).any()


def test_the_twin_runs_clean_under_the_host_sanitizers():
    """tests/host/embed_topk_twin_main.cpp with w2b_embed_twins.cpp alone, built with ASan and UBSan by `make host-check`'s
    target and run once, as its five siblings are"""
    csrc = os.path.join(ROOT, "word2bits_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "build/embed_topk_twin_check"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(csrc, "build", "embed_topk_twin_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.fullmatch(r"w2b_embed_topk_host: \d+ calls ok, \d+ refused\n", out.stdout), out.stdout
