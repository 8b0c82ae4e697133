"""The packed embedding's softmax cross-entropy (include/word2bits_embed.h, "Cross-entropy"), the part that needs no GPU:
the ABI, expneg and its accuracy, the host twin against an independent numpy restatement (bit for bit), the consequences
the header states, loss and gradient against torch in float64 within a bound derived below, every refusal with its cause,
and the stand-alone sanitizer program of the twin."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT
from test_embed_host import make_table, same_bits
from test_embed_project_host import host_project, round_f32, wide_values
from test_embed_backproject_host import cand_list, host_backproject

SYMBOLS = {"w2b_embed_xent": "int", "w2b_embed_reserve_xent": "int", "w2b_embed_xent_device": "int",
           "w2b_embed_xent_host": "int", "w2b_embed_expneg_host": "float"}
ROWS = 300
XSEG = 256
MS = [1, 2, 255, 256, 257, 1025, 2500]
EXPNEG_ULPS = 1.0            # asserted below: the next whole ulp above the 0.881 ulp measured on the dense sample
U = 2.0 ** -24               # one float32 rounding, relative


def expneg(r):
    return np.float32(_lib.lib().w2b_embed_expneg_host(float(np.float32(r))))


def mild_values(rng, shape):
    """multiples of 1/64 in [-1/4, 1/4]: logits a few units apart up to dim 200, so that every probability is far above
    2^-60 (the g of such a call passes the value rule of w2b_embed_backproject_host), and every partial sum of a chain is
    an integer below 2^24 times 2^-6: exact"""
    return (rng.integers(-16, 17, shape) / 64.0).astype(np.float32)


def host_xent(packed, dim, bitlevel, x, cand, target, grad=True, n=None, m=None, rows=None):
    """w2b_embed_xent_host: (rc, mx, se, tl, dx), the outputs filled with NaN before the call"""
    x = None if x is None else np.ascontiguousarray(x, np.float32)
    cand = None if cand is None else np.ascontiguousarray(cand, np.int32)
    target = None if target is None else np.ascontiguousarray(target, np.int32)
    n = (0 if x is None else x.size // dim) if n is None else n
    m = (packed.shape[0] if cand is None else cand.size) if m is None else m
    out = [np.full(max(n, 0), np.nan, np.float32) for _ in range(3)]
    dx = np.full((max(n, 0), dim), np.nan, np.float32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    rc = _lib.lib().w2b_embed_xent_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0] if rows is None else rows, dim,
                                        bitlevel, n, ptr(x, _lib.f32p), m, ptr(cand, _lib.i32p), ptr(target, _lib.i32p),
                                        *[ptr(o, _lib.f32p) for o in out], ptr(dx, _lib.f32p) if grad else None)
    return (rc, *out, dx)


def targets_for(rng, cand, m, n):
    """live target positions: the first and the last live one, one per 64 candidates further on (another wavefront's
    range), a repeated row where the list has one, random ones; vector 1 (if there is one) is ignored"""
    live = np.arange(m) if cand is None else np.flatnonzero(cand >= 0)
    t = rng.choice(live, n)
    picks = [live[0], live[-1], live[min(len(live) - 1, 70)], live[min(len(live) - 1, 200)]]
    if cand is not None and m >= 9:
        picks.append(6)                                   # cand[5] == cand[6] == cand[2] in cand_list
    for k, p in enumerate(picks):
        if 2 + k < n:
            t[2 + k] = p
    if n == 1:
        t[0] = live[-1]
    if n > 1:
        t[0], t[1] = live[0], -1
    return t.astype(np.int32)


def fma32(a, b, c):
    """fmaf(a, b, c) of three float32, exactly: the rational a * b + c rounded once.  (Through float64 the sum would be
    rounded twice: a term u * e may lie 2^-100 below se, far outside 53 bits.)"""
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def numpy_xent(l, cand, target):
    """the header's steps 2 to 5 for one vector, independently of the twin's loops: l = the projection's float32 logits [m];
    segments by slicing, U_s in Python integers, se by exact fused steps.  Returns mx, se, tl, the list of U_s and g."""
    m = len(l)
    live = np.ones(m, bool) if cand is None else cand >= 0
    Ms, Us = [], []
    for j0 in range(0, m, XSEG):
        ls = l[j0:j0 + XSEG][live[j0:j0 + XSEG]]
        if len(ls) == 0:
            continue
        M = ls.max()
        d = ls - M                                        # float32 - float32: one rounding each
        assert d.dtype == np.float32
        terms = [int(np.rint(np.float64(expneg(v)) * 2.0 ** 32)) for v in d]
        assert all(0 <= t <= 2 ** 32 for t in terms)
        Ms.append(M)
        Us.append(sum(terms))
    mx = max(Ms) if Ms else np.float32(0)
    se = np.float32(0)
    for M, Uint in zip(Ms, Us):
        uf = np.float32(Uint)                             # < 2^53: exact in float64, then rounded once to float32
        se = fma32(uf * np.float32(2.0 ** -32), expneg(M - mx), se)
    tl = l[target] if target >= 0 else np.float32(0)
    g = np.zeros(m, np.float32)
    if target >= 0:
        e = np.array([expneg(v) for v in (l - mx)], np.float32)
        g = np.where(live, e / se, np.float32(0)).astype(np.float32)
        g[target] = g[target] - np.float32(1)
    return np.float32(mx), np.float32(se), np.float32(tl), Us, g


def test_abi_is_exported_declared_and_bound():
    lib = C.CDLL(os.path.join(ROOT, "word2bits_amd", "libword2bits_hip.so"))
    header = open(os.path.join(ROOT, "include", "word2bits_embed.h")).read()
    for name, res in SYMBOLS.items():
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is (C.c_int if res == "int" else C.c_float), name
        assert re.search(r"^%s\s*%s\(" % (res, name), header, flags=re.M), name
    for method in ("xent", "reserve_xent", "xent_device", "staging_xent", "torch_xent"):
        assert callable(getattr(w2b.PackedEmbedding, method, None)), method
    assert re.search(r"#define\s+W2B_EMBED_XSEG\s+256\b", header)
    assert "Cross-entropy (w2b_embed_xent*" in header


def test_expneg_is_exact_where_the_header_says_so():
    assert expneg(0.0).view(np.uint32) == 0x3F800000 and expneg(-0.0).view(np.uint32) == 0x3F800000
    below = np.nextafter(np.float32(-64), np.float32(-np.inf))
    for r in (below, -65.0, -100.0, -1e30, -np.inf, np.nan):
        assert expneg(r).view(np.uint32) == 0, r          # +0.0 exactly
    tiny = np.float32(np.finfo(np.float32).tiny)
    for r in (-64.0, -63.999996, -63.5, -1e-30, -1e-45):
        v = expneg(r)
        assert tiny <= 2.0 ** -93 <= v <= 1.0, r          # normal, and never above 1
    # the constants of the header: 1 / i! and the split of ln 2, rounded to float32
    src = open(os.path.join(ROOT, "word2bits_amd", "csrc", "w2b_embed_shared.h")).read()
    const = {k: int(v, 16) for k, v in re.findall(r"#define W2B_XENT_(\w+) (0x[0-9A-Fa-f]+)u", src)}
    f32 = lambda v: int(np.float32(v).view(np.uint32))
    assert const["LOG2E"] == f32(math.log2(math.e)) and all(const["C%d" % i] == f32(1.0 / math.factorial(i)) for i in range(2, 8))
    hi = float(np.uint32(const["LN2_HI"]).view(np.float32))
    assert const["LN2_LO"] == f32(math.log(2) - hi) and const["LN2_HI"] & 0x1FF == 0


def dense_sample():
    """every 509th float32 pattern of [-64, -2^-20], and the 17 patterns around every multiple of ln2 / 2 (where k changes)"""
    lo, hi = 0xB5800000, 0xC2800000
    bits = [np.arange(lo, hi + 1, 509, dtype=np.uint64).astype(np.uint32)]
    for k in range(1, 186):
        b = int(np.float32(-k * math.log(2) / 2).view(np.uint32))
        bits.append(np.arange(max(lo, b - 8), min(hi, b + 8) + 1, dtype=np.uint64).astype(np.uint32))
    return np.concatenate(bits).view(np.float32)


def test_expneg_is_within_one_ulp_of_exp_on_a_dense_sample():
    """Against numpy's float64 exp (whose own error, 2^-52 relative, is 2^-29 ulp here).  Measured on this sample: 0.881 ulp
    at r = -16.978045; asserted: the next whole ulp, EXPNEG_ULPS = 1, which is also what the bounds below use (a relative
    error of at most 2^-23).  Every result is a normal number no greater than 1."""
    r = dense_sample()
    f = _lib.lib().w2b_embed_expneg_host
    got = np.array([f(float(v)) for v in r], np.float32)
    want = np.exp(r.astype(np.float64))
    ulp = 2.0 ** (np.floor(np.log2(want)) - 23)
    err = np.abs(got.astype(np.float64) - want) / ulp
    print("expneg: %d points, largest error %.4f ulp at r = %r" % (len(r), err.max(), r[err.argmax()]))
    assert len(r) > 400_000 and err.max() < EXPNEG_ULPS
    assert (got <= 1).all() and (got >= 2.0 ** -93).all()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 65, 200])
def test_twin_equals_the_numpy_restatement(dim, bitlevel):
    """mild x (probabilities of ordinary size) and x over the whole allowed range (logits 2^80 apart: the exact-zero branch,
    segments whose U_s is scaled to nothing); with candidates and with every row; mx, se, tl, and dx through the twin of
    the back-projection applied to the restatement's g.  That twin refuses a g below 2^-60, which the mild x never produce
    and the wide x hardly ever (their probabilities are 1, 0, or shared between equal logits): a vector whose g it would
    refuse is left out of the dx comparison"""
    rng = np.random.default_rng(300 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    n = 4
    for m in MS + [None]:
        cand = None if m is None else cand_list(rng, ROWS, m)
        if cand is not None and m < 9:
            cand[:] = np.abs(cand)
        mm = ROWS if m is None else m
        for mild, x in ((True, mild_values(rng, (n, dim))), (False, wide_values(rng, (n, dim)))):
            target = targets_for(rng, cand, mm, n)
            rc, mx, se, tl, dx = host_xent(packed, dim, bitlevel, x, cand, target)
            assert rc == 0, _lib.lib().w2b_last_error()
            rc, l = host_project(packed, dim, bitlevel, x, cand)
            assert rc == 0
            G = np.zeros((n, mm), np.float32)
            for i in range(n):
                wmx, wse, wtl, _, G[i] = numpy_xent(l[i], cand, int(target[i]))
                assert (mx[i].view(np.uint32), se[i].view(np.uint32), tl[i].view(np.uint32)) == \
                    (wmx.view(np.uint32), wse.view(np.uint32), wtl.view(np.uint32)), (m, i)
            admitted = ~((G != 0) & (np.abs(G) < 2.0 ** -60)).any(axis=1)
            assert admitted.all() or not mild, m
            rc, want = host_backproject(packed, dim, bitlevel, G[admitted], cand)
            assert rc == 0 and same_bits(dx[admitted], want), m


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_the_consequences_the_header_states(bitlevel):
    rng = np.random.default_rng(90 + bitlevel)
    dim, n, m = 65, 5, 1025
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    cand = cand_list(rng, ROWS, m)
    x = mild_values(rng, (n, dim))
    target = targets_for(rng, cand, m, n)
    rc, mx, se, tl, dx = host_xent(packed, dim, bitlevel, x, cand, target)
    rc2, l = host_project(packed, dim, bitlevel, x, cand)
    assert rc == 0 and rc2 == 0
    # (a) mx and tl are logits of the projection's twin
    live = cand >= 0
    assert same_bits(mx, l[:, live].max(axis=1))
    assert same_bits(tl, np.where(target >= 0, l[np.arange(n), np.maximum(target, 0)], np.float32(0)).astype(np.float32))
    assert tl[1].view(np.uint32) == 0 and not dx[1].view(np.uint32).any()        # the ignored vector: +0.0
    # (b) dx is the back-projection's twin applied to the g of step 5
    G = np.stack([numpy_xent(l[i], cand, int(target[i]))[4] for i in range(n)])
    rc, want = host_backproject(packed, dim, bitlevel, G, cand)
    assert rc == 0 and same_bits(dx, want) and np.abs(dx).max() > 0
    # no gradient asked for: the same statistics
    rc, mx2, se2, tl2, dx2 = host_xent(packed, dim, bitlevel, x, cand, target, grad=False)
    assert rc == 0 and same_bits(mx2, mx) and same_bits(se2, se) and same_bits(tl2, tl) and np.isnan(dx2).all()
    # (c) a permutation within the segments changes neither mx, nor se, nor any U_s (and does change dx's chains)
    perm = np.concatenate([j0 + rng.permutation(min(XSEG, m - j0)) for j0 in range(0, m, XSEG)])
    inv = np.argsort(perm)
    tp = np.where(target >= 0, inv[np.maximum(target, 0)], -1).astype(np.int32)
    rc, mxp, sep, tlp, _ = host_xent(packed, dim, bitlevel, x, cand[perm], tp)
    assert rc == 0 and same_bits(mxp, mx) and same_bits(sep, se) and same_bits(tlp, tl)
    for i in (0, 2):
        assert numpy_xent(l[i][perm], cand[perm], int(tp[i]))[3] == numpy_xent(l[i], cand, int(target[i]))[3]
    # (d) a padding-only segment, in front or behind, changes nothing
    pad = np.full(XSEG, -1, np.int32)
    rc, mxd, sed, tld, dxd = host_xent(packed, dim, bitlevel, x, np.concatenate([cand, pad, pad]), target)
    assert rc == 0 and same_bits(mxd, mx) and same_bits(sed, se) and same_bits(tld, tl)
    shifted = np.where(target >= 0, target + XSEG, -1).astype(np.int32)
    rc, mxd, sed, tld, _ = host_xent(packed, dim, bitlevel, x, np.concatenate([pad, cand]), shifted)
    assert rc == 0 and same_bits(mxd, mx) and same_bits(sed, se) and same_bits(tld, tl)
    # (e) one candidate, target 0
    rc, mx1, se1, tl1, dx1 = host_xent(packed, dim, bitlevel, x, cand[1:2], np.zeros(n, np.int32))
    assert rc == 0 and same_bits(mx1, tl1) and (se1.view(np.uint32) == 0x3F800000).all() and not dx1.view(np.uint32).any()
    # nothing live: mx = se = +0.0, and only an ignored vector is accepted
    rc, mx0, se0, tl0, dx0 = host_xent(packed, dim, bitlevel, x, pad, np.full(n, -1, np.int32))
    assert rc == 0 and not any(a.view(np.uint32).any() for a in (mx0, se0, tl0, dx0))
    rc, mx0, se0, tl0, dx0 = host_xent(packed, dim, bitlevel, x, np.zeros(0, np.int32), np.full(n, -1, np.int32))
    assert rc == 0 and not any(a.view(np.uint32).any() for a in (mx0, se0, tl0, dx0))


def bounds(m, bitlevel, lmax):
    """The bounds of the comparison with float64, from the definition alone.  u = 2^-24 (one rounding), expneg within
    EXPNEG_ULPS ulp = 2 u relative, nseg = ceil(m / 256), every term of se positive.
    se.  A term exp(l - M_s): the float32 difference is off by |d| u <= 64 u (larger differences give 0: each such term is
      below e^-64 of the largest, m e^-64 in all, nothing), expneg by 2 u; its integer by 2^-33 absolute, so a segment's
      U_s 2^-32 by 256 x 2^-33 = u / 2 relative to its largest term, which is 1; (float)U_s by u; expneg(M_s - mx) by
      64 u + 2 u again; the nseg fused adds by u each of a growing positive sum.  rho = (66 + 0.5 + 1 + 66 + nseg) u.
    loss = (mx - tl) + log(se) in float64: |d loss| <= rho (log(1 + rho) <= rho), plus 2^-50 of |mx - tl| for float64.
    g.  p_j = expneg(l_j - mx) / se: 64 u + 2 u, rho, and u for the division: rho_g = rho + 67 u relative; the target's
      "- 1" rounds once more, u absolute.  Sum over j of |delta g_j| <= rho_g + u since the p_j sum to 1.
    dx[a] = q sum_j g_j t_j[a] by chains of at most 1024 fmaf, ceil(m / 1024) adds and one multiply: (min(m, 1024) +
      ceil(m / 1024) + 1) u relative to sum_j |g_j| |q t_j| <= 2 vmax (the p_j sum to 1, the target adds |p_t - 1| <= 1),
      vmax = 0.75 or 1/3 the largest |table value|.
    At bitlevel 1 the reference's logits are x . table in float64, where q = 0x3EAAAAAB enters exactly, and ours round S q
    once: every logit is off by at most u lmax, which moves logsumexp and tl by that much each (loss: 2 u lmax) and every p_j
    by at most 2 u lmax relative.  At bitlevel 2 with the mild x both are exact.  1.01 covers the second-order terms."""
    nseg = -(-m // XSEG)
    rho = (133.5 + nseg) * U
    shift = 2 * U * lmax if bitlevel == 1 else 0.0
    vmax = 1.0 / 3 + 1e-7 if bitlevel == 1 else 0.75
    loss = 1.01 * (rho + shift) + 2.0 ** -50 * 2 * lmax
    dx = 1.01 * vmax * ((rho + 67 * U + shift + U) + 2 * (min(m, 1024) + -(-m // 1024) + 1) * U)
    return loss, dx


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_loss_and_gradient_against_torch_in_float64(bitlevel):
    """torch.nn.functional.cross_entropy on float64 logits x @ table[cand].T (padding columns masked to -inf) and its
    autograd, on the CPU; the bound is bounds() above, derived from m, the expneg bound and 2^-24, not from a run"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(70 + bitlevel)
    dim, n = 200, 6
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    W = torch.from_numpy(table).double()
    for m in (257, 2500, None):
        cand = None if m is None else cand_list(rng, ROWS, m)
        mm = ROWS if m is None else m
        x = mild_values(rng, (n, dim))
        target = targets_for(rng, cand, mm, n)
        rc, mx, se, tl, dx = host_xent(packed, dim, bitlevel, x, cand, target)
        assert rc == 0
        ours = np.where(target >= 0, (mx.astype(np.float64) - tl) + np.log(se.astype(np.float64)), 0.0)
        xt = torch.from_numpy(x).double().requires_grad_()
        logits = xt @ (W if cand is None else W[torch.from_numpy(np.maximum(cand, 0)).long()]).T
        if cand is not None:
            logits = logits.masked_fill(torch.from_numpy(cand < 0), float("-inf"))
        ref = F.cross_entropy(logits, torch.from_numpy(target).long(), ignore_index=-1, reduction="none")
        ref.sum().backward()
        lmax = float(logits.detach()[torch.isfinite(logits.detach())].abs().max())
        b_loss, b_dx = bounds(mm, bitlevel, lmax)
        e_loss = float(np.abs(ours - ref.detach().numpy()).max())
        e_dx = float(np.abs(dx.astype(np.float64) - xt.grad.numpy()).max())
        print("m = %s bitlevel %d: loss off by %.3g (bound %.3g), dx off by %.3g (bound %.3g)" % (m, bitlevel, e_loss, b_loss, e_dx, b_dx))
        assert e_loss <= b_loss and e_dx <= b_dx and ref.detach().abs().max() > 1


def test_every_refusal_names_its_cause_and_leaves_the_outputs_untouched():
    rng = np.random.default_rng(8)
    dim, bitlevel = 65, 2
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    L = _lib.lib()
    err = lambda: L.w2b_last_error().decode()
    cand = cand_list(rng, ROWS, 9)                                            # padding at 0, 4 and 8
    x = wide_values(rng, (4, dim))
    target = np.array([1, -1, 7, 3], np.int32)

    def refused(res, *words, code=_lib.W2B_EINVAL):
        rc, *outs = res
        assert rc == code and all(w in err() for w in words), (rc, err())
        assert all(np.isnan(o).all() for o in outs)

    rc, *outs = host_xent(packed, dim, bitlevel, x, cand, target)
    assert rc == 0 and not any(np.isnan(o).any() for o in outs)
    # 1. what needs no handle / no table
    refused(host_xent(packed, dim, bitlevel, x, cand, target, n=-1), "vector count")
    refused(host_xent(packed, dim, bitlevel, x, cand, target, n=(1 << 24) + 1), "vector count")
    refused(host_xent(packed, dim, bitlevel, x, cand, target, m=-1), "candidate count")
    refused(host_xent(packed, dim, bitlevel, None, cand, target, n=4), "null vectors")
    refused(host_xent(packed, dim, bitlevel, x, cand, None), "null targets")
    a = (packed.ctypes.data_as(_lib.u64p), ROWS, dim, bitlevel, 4, x.ctypes.data_as(_lib.f32p), 9, cand.ctypes.data_as(_lib.i32p),
         target.ctypes.data_as(_lib.i32p))
    o = [np.full(4, np.nan, np.float32) for _ in range(3)]
    op = [v.ctypes.data_as(_lib.f32p) for v in o]
    for k in range(3):
        args = list(op)
        args[k] = None
        assert L.w2b_embed_xent_host(*a, *args, None) == _lib.W2B_EINVAL and "null output" in err()
    # 2. the table
    assert L.w2b_embed_xent_host(None, *a[1:], *op, None) == _lib.W2B_EINVAL and "null table" in err()
    assert L.w2b_embed_xent_host(a[0], ROWS, dim, 3, *a[4:], *op, None) == _lib.W2B_EUNSUPPORTED and "bitlevel" in err()
    assert all(np.isnan(v).all() for v in o)
    # 3. the candidates, 4. the targets, 5. the values: each before the next
    c = cand.copy()
    c[5] = ROWS
    bad_t, bad_x = target.copy(), x.copy()
    bad_t[2], bad_x[0, 3] = 9, np.nan
    refused(host_xent(packed, dim, bitlevel, bad_x, c, bad_t), "cand[5]", "rows")
    refused(host_xent(packed, dim, bitlevel, x, None, target, m=ROWS - 1), "must be rows")
    refused(host_xent(packed, dim, bitlevel, bad_x, cand, bad_t), "vector 2", "target 9", "m = 9")
    bad_t[2], bad_t[3] = 7, 4
    refused(host_xent(packed, dim, bitlevel, bad_x, cand, bad_t), "vector 3", "target 4", "padding")
    refused(host_xent(packed, dim, bitlevel, x, np.zeros(0, np.int32), np.zeros(4, np.int32)), "vector 0", "target 0")
    refused(host_xent(packed, dim, bitlevel, bad_x, cand, target), "vector 0", "column 3")
    for v in (np.inf, 2.0 ** 61, -(2.0 ** -61), 1e-45):
        y = x.copy()
        y[3, 64] = v
        refused(host_xent(packed, dim, bitlevel, y, cand, target), "vector 3", "column 64")
    # n == 0 is fine, with or without pointers
    assert host_xent(packed, dim, bitlevel, None, cand, None, n=0)[0] == 0
    # the host form: what needs no handle comes first, so it is refused without a device and without a handle
    form = lambda n, xp, m, cp, tp, outs, h=None: L.w2b_embed_xent(h, n, xp, m, cp, tp, *outs, None)
    xp, cp, tp = a[5], a[7], a[8]
    assert form(-1, xp, 9, cp, tp, op) == _lib.W2B_EINVAL and "vector count" in err()
    assert form(4, xp, 0x7FFFFF01, cp, tp, op) == _lib.W2B_EINVAL and "candidate count" in err()
    assert form(4, None, 9, cp, tp, op) == _lib.W2B_EINVAL and "null vectors" in err()
    assert form(4, xp, 9, cp, None, op) == _lib.W2B_EINVAL and "null targets" in err()
    assert form(4, xp, 9, cp, tp, [op[0], None, op[2]]) == _lib.W2B_EINVAL and "null output" in err()
    assert form(4, xp, 9, cp, tp, op) == _lib.W2B_EINVAL and "null handle" in err()
    assert L.w2b_embed_reserve_xent(None, 1, 1, None, None, None, None, None) == _lib.W2B_EINVAL
    assert L.w2b_embed_xent_device(None, 1, 1, 1, 0) == _lib.W2B_EINVAL
    assert all(np.isnan(v).all() for v in o)


def test_the_twin_runs_clean_under_the_host_sanitizers():
    """tests/host/embed_xent_twin_main.cpp with w2b_embed_twins.cpp, built with -fsanitize=address,undefined as a program of
    its own (the Makefile's host-check target for it) and run once: no library, no Python, no GPU under the sanitizer"""
    csrc = os.path.join(ROOT, "word2bits_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "build/embed_xent_twin_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(csrc, "build", "embed_xent_twin_check")], capture_output=True, text=True,
                       stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and r.stderr == "" and re.search(r"w2b_embed_xent_host: \d+ calls ok, \d+ refused", r.stdout), \
        r.stdout + r.stderr
