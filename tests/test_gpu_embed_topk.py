"""The packed embedding's top-k selection on the GPU (include/word2bits_embed.h, "Top-k"): the host form, the device form by
hand and the device form with slack in the reserve against the host twin of tests/test_embed_topk_host.py (which ties it to
the projection's twin and a stable sort), without a tolerance; the ranges of vectors; what the device form does with bad
inputs; the torch fronts.  The inputs, and the proof that each kind reaches the branch it is meant for, are in that file
(case(), test_the_kinds_of_input_reach_the_branches_they_are_meant_for).  The only tolerance is on log_probs, whose
logarithm is outside the contract."""
import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from test_embed_host import make_table
from test_embed_project_host import host_project
from test_embed_topk_host import KS, MAX_K, ROWS, case, topk_cands, twin, x_gauss
from test_gpu_embed import same

pytestmark = pytest.mark.gpu
DIMS = [1, 33, 64, 65, 200, 513]
NS = [1, 33, 65, 130]
SCRATCH = "W2B_EMBED_TOPK_SCRATCH"       # the library's override of the bytes of selection scratch per range of vectors


def host_form(emb, x, cand, k):
    """w2b_embed_topk through ctypes: (vals, pos int32), NaN / -77 before the call"""
    n = len(x)
    x = np.ascontiguousarray(x, np.float32)
    cand = None if cand is None else np.ascontiguousarray(cand, np.int32)
    vals, pos = np.full((n, k), np.nan, np.float32), np.full((n, k), -77, np.int32)
    _lib.check(emb._L.w2b_embed_topk(emb._h, n, x.ctypes.data_as(_lib.f32p), emb.rows if cand is None else cand.size,
                                     None if cand is None else cand.ctypes.data_as(_lib.i32p), k, vals.ctypes.data_as(_lib.f32p),
                                     pos.ctypes.data_as(_lib.i32p)))
    return vals, pos


def device_form(emb, x, cand, k, slack=0):
    """the device form by hand: reserve (`slack` more of everything), fill the staging views, launch, synchronise, read:
    (vals, pos int64) as tensors, dense [n, k]"""
    import torch
    n, m = len(x), emb.rows if cand is None else len(cand)
    max_k = min(MAX_K, k + slack)
    x_t, cand_t, vals, pos = emb.staging_topk(n + slack, m + slack, max_k)
    assert x_t.shape == (n + slack, emb.dim) and cand_t.dtype == torch.int64 and cand_t.shape == (m + slack,)
    assert vals.shape == pos.shape == ((n + slack) * max_k,) and pos.dtype == torch.int64 and vals.is_cuda and pos.is_cuda
    x_t[:n].copy_(torch.from_numpy(np.array(x, np.float32)))
    if cand is not None:
        cand_t[:m].copy_(torch.from_numpy(np.array(cand, np.int64)))
    vals.fill_(float("nan"))
    pos.fill_(-77)
    torch.cuda.synchronize()
    emb.topk_device(n, m, k, cand is not None)
    emb.synchronize()
    if slack:
        assert torch.isnan(vals[n * k:]).all() and (pos[n * k:] == -77).all()      # dense for the n and k of the call
    return vals[:n * k].view(n, k).clone(), pos[:n * k].view(n, k).clone()


def equal(got, want, n, k, tag):
    vals, pos = got
    pos = pos.cpu().numpy() if hasattr(pos, "cpu") else pos
    assert same(vals, np.ascontiguousarray(want[0][:n, :k]), "float32"), (tag, "vals")
    assert np.array_equal(pos, want[1][:n, :k]), (tag, "pos")


def run_entries(emb, entries, ns, ks):
    """every n of ns x every k of ks in the device form; the host form and the device form with slack at one (n, k) per
    entry, walking through ns and ks from entry to entry, and at the largest of both"""
    for idx, (name, cand, x, want) in enumerate(entries):
        mine = sorted({min(n, len(x)) for n in ns})
        for n in mine:
            xn = np.ascontiguousarray(x[:n])
            for k in ks:
                equal(device_form(emb, xn, cand, k), want, n, k, (name, None if cand is None else len(cand), n, k, "device form"))
        for n, k in {(mine[idx % len(mine)], ks[idx % len(ks)]), (mine[-1], ks[-1])}:
            xn = np.ascontiguousarray(x[:n])
            tag = (name, None if cand is None else len(cand), n, k)
            equal(host_form(emb, xn, cand, k), want, n, k, (tag, "host form"))
            equal(device_form(emb, xn, cand, k, slack=7), want, n, k, (tag, "device form with slack"))


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", DIMS)
def test_every_form_equals_the_twin(gpu, dim, bitlevel):
    """300 rows: every candidate list (m of 1, 2, 255, 256, 257, 1025, 2500 and all rows; sparse; near-duplicates) x its sets
    of vectors x n of 1, 33, 65, 130 x k of 1, 2, 31, 32, 33, 64; then all 2100 rows of a second table (33 units, the last
    partial).  dim 513 walks the chunked K loop."""
    packed, table, lists, big, wide = case(dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    run_entries(emb, lists, NS, KS)
    assert emb.bad_ids() == 0
    # the numpy front: any shape
    name, cand, x, want = lists[3 * 5]                                        # m = 1025, gauss
    vals, pos = emb.topk(x[:6].reshape(2, 3, dim), 5, cand)
    assert vals.shape == pos.shape == (2, 3, 5) and vals.dtype == np.float32 and pos.dtype == np.int32
    equal((vals.reshape(6, 5), pos.reshape(6, 5)), want, 6, 5, "numpy front")
    emb.close()
    emb = w2b.PackedEmbedding(packed=big, dim=dim, bitlevel=bitlevel)
    run_entries(emb, wide, (1, 130), (1, 33, 64))
    emb.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_ranges_of_vectors_give_the_same_bits(gpu, monkeypatch, bitlevel):
    """A call whose unit maxima and key lists do not fit the scratch runs in ranges of vectors, never fewer than 64 (one pair
    of tiles).  With W2B_EMBED_TOPK_SCRATCH at one byte, 130 vectors are three ranges (64, 64, 2): three selection launches
    instead of one, the same bits, and the twin's."""
    dim = 200
    packed, table, lists, _, _ = case(dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    for name, cand, x, want in lists:
        if name != "gauss" or (cand is not None and len(cand) not in (257, 2500)):
            continue
        for k in (1, 33, 64):
            monkeypatch.delenv(SCRATCH, raising=False)
            emb.timing()
            whole = device_form(emb, x, cand, k)
            assert emb.timing()[1] == 1
            monkeypatch.setenv(SCRATCH, "1")
            ranged = device_form(emb, x, cand, k)
            assert emb.timing()[1] == 3
            assert same(ranged[0], whole[0].cpu().numpy(), "float32") and (ranged[1] == whole[1]).all()
            equal(ranged, want, len(x), k, (name, k, "ranges"))
            equal(host_form(emb, x, cand, k), want, len(x), k, (name, k, "host form, ranges"))
            assert emb.timing()[1] == 3
    emb.close()


def test_device_form_never_answers_with_a_dead_candidate_and_counts_the_refused(gpu):
    """candidates >= rows and < 0 written into the staging (reserved a little larger, so that even an unclamped access would
    stay inside the allocations): never an answer; each refused one counted once per call, whatever n and the ranges are"""
    rng = np.random.default_rng(53)
    dim, bitlevel, n, m = 200, 2, 70, 1500
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    cand = rng.integers(0, ROWS, m).astype(np.int64)
    cand[[3, 77, 1000]] = -1, -9, -(1 << 40)
    bad = [17, 64, 1400, 1499]
    plant = cand.copy()
    plant[bad] = ROWS, ROWS + 5, 1 << 40, 2 ** 31
    clean = cand.copy()
    clean[bad] = -1
    clean[1000] = -1
    x = x_gauss(rng, n, dim)
    want = twin(packed, dim, bitlevel, x, clean.astype(np.int32))
    dead = np.flatnonzero(clean < 0)
    for k in (1, 64):
        got = device_form(emb, x, plant, k, slack=64)
        equal(got, want, n, k, ("bad inputs", k))
        assert not np.isin(got[1].cpu().numpy(), dead).any()
        assert emb.bad_ids() == len(bad) and emb.bad_ids() == 0
    import torch
    with pytest.raises(w2b.W2bError) as e:
        emb.torch_topk(torch.from_numpy(np.array(x)), 5, torch.from_numpy(plant))
    assert e.value.code == _lib.W2B_EINVAL and emb.bad_ids() == 0
    # the host form refuses before any launch, in the stated order; the outputs stay untouched
    emb.timing()
    for args, cause in (((x[:1], np.array([1, ROWS], np.int32), 1), "cand[1]"), ((x[:1], None, 0), "k = 0"),
                        ((x[:1], None, 65), "k = 65"), ((np.full((1, dim), np.inf, np.float32), None, 1), "vector 0, column 0")):
        with pytest.raises(w2b.W2bError) as e:
            host_form(emb, *args)
        assert e.value.code == _lib.W2B_EINVAL and cause in str(e.value), cause
    assert emb.timing()[1] == 0
    # nothing live, and m == 0: empty lists
    pad = np.full(300, -1, np.int64)
    for c in (pad, pad[:0]):
        vals, pos = device_form(emb, x[:5], c, 3)
        assert (pos == -1).all() and (vals.view(torch.int32) == -8388608).all()
    vals, pos = host_form(emb, x[:5], np.zeros(0, np.int32), 3)
    assert (pos == -1).all() and (vals.view(np.uint32) == 0xFF800000).all()
    assert emb.topk(np.zeros((0, dim), np.float32), 3)[0].shape == (0, 3) and emb.bad_ids() == 0
    emb.close()


def test_reserve_keeps_its_pointers_and_the_other_calls_are_not_disturbed(gpu):
    import torch
    from test_embed_host import ref_bag
    from test_embed_backproject_host import host_backproject
    from test_embed_project_host import wide_values
    rng = np.random.default_rng(59)
    dim, bitlevel, m = 65, 1, 700
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    cand = topk_cands(rng, ROWS, m)
    x = wide_values(rng, (33, dim))
    g = wide_values(rng, (33, m))
    ids = rng.integers(0, ROWS, 90).astype(np.int32)
    offsets = np.array([0, 10, 10, 90], np.int64)
    rc, want_p = host_project(packed, dim, bitlevel, x, cand)
    rc2, want_b = host_backproject(packed, dim, bitlevel, g, cand)
    assert rc == 0 and rc2 == 0
    want_bag = ref_bag(table, bitlevel, ids, offsets, "sum")
    want = twin(packed, dim, bitlevel, x, cand)

    def others():
        ct = torch.from_numpy(np.array(cand))
        assert same(emb.torch_project(torch.from_numpy(np.array(x)), ct), want_p, "float32")
        assert same(emb.torch_backproject(torch.from_numpy(np.array(g)), ct), want_b, "float32")
        assert same(emb.torch_bag(torch.from_numpy(ids), torch.from_numpy(offsets), "sum"), want_bag, "float32")

    others()
    views = (emb.torch_project(torch.from_numpy(np.array(x)), torch.from_numpy(np.array(cand)), copy=False),
             emb.torch_backproject(torch.from_numpy(np.array(g)), torch.from_numpy(np.array(cand)), copy=False))
    equal(device_form(emb, x, cand, 33), want, 33, 33, "between")
    assert same(views[0], want_p, "float32") and same(views[1], want_b, "float32")       # the views of their buffers still hold
    others()
    # buffers of its own: growing the others leaves them, growing them leaves the others
    rest = (emb.reserve(50, 2), emb.reserve_weights(50), emb.reserve_project(4, 10), emb.reserve_backproject(4, 10),
            emb.reserve_xent(4, 10))
    small = emb.reserve_topk(33, 700, 33)
    assert emb.reserve_topk(2, 5, 1) == small and len(small) == 4 and len(set(small)) == 4
    grown = emb.reserve_topk(33, 2000, 33)                                    # more candidates: only cand_dev may move
    assert (grown[0], grown[2], grown[3]) == (small[0], small[2], small[3])
    assert (emb.reserve(50, 2), emb.reserve_weights(50), emb.reserve_project(4, 10), emb.reserve_backproject(4, 10),
            emb.reserve_xent(4, 10)) == rest
    emb.reserve(5000, 100)
    emb.reserve_project(50, 400)
    emb.reserve_xent(50, 400)
    assert emb.reserve_topk(33, 2000, 33) == grown
    for args in ((34, 5, 1), (5, 2001, 1), (-1, 5, 1), (5, -1, 1), (33, 5, 34), (5, 5, 0), (5, 5, 65)):
        with pytest.raises(w2b.W2bError) as e:
            emb.topk_device(*args)
        assert e.value.code == _lib.W2B_EINVAL, args
    emb.topk_device(17, 5, 64)                                               # n x k within what was reserved
    emb.synchronize()
    with pytest.raises(w2b.W2bError) as e:
        emb.topk_device(5, 2000, 1, False)                                   # all rows: m must be rows
    assert e.value.code == _lib.W2B_EINVAL
    with pytest.raises(w2b.W2bError):
        emb.reserve_topk(5, 5, 65)
    fresh = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    with pytest.raises(w2b.W2bError):
        fresh.topk_device(1, 1, 1)                                           # nothing reserved
    fresh.close()
    emb.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_torch_topk_is_torch_topk_of_the_projection(gpu, bitlevel):
    """On the gaussian vectors against 2100 random rows -- no tie among the 64 best, asserted on the twin in the host test --
    torch_topk equals torch.topk(torch_project(x), k): the values bit for bit, and the indices; the same through a candidate
    list of distinct rows, from vectors of any shape and dtype on any device; nothing is recorded for autograd.
    log_probs=True is values - logsumexp(torch_project(x)) within a tolerance.  The issue sets 1e-5 relative, "the float32 log
    plus one subtraction"; the xent test records no figure to take four times.  Relative to what: both sides subtract
    numbers of the size of the logits and of the logsumexp, and torch's logsumexp is itself a float32 sum and a float32
    log at that size, so each rounding is 2^-24 of max(|logit|, |logsumexp|), not of the difference, which for a dominant
    answer is close to 0.  The bound is therefore 1e-5 x the largest |logit| or |logsumexp| of the call.  The largest
    difference seen is printed; DESIGN.md 3.6 records it."""
    import torch
    dim = 200
    packed, table, lists, big, wide = case(dim, bitlevel)
    name, cand, x, want = wide[0]
    emb = w2b.PackedEmbedding(packed=big, dim=dim, bitlevel=bitlevel)
    xt = torch.from_numpy(np.array(x))
    rows = torch.from_numpy(np.random.default_rng(61).permutation(2100)[:1025].astype(np.int64))
    for ct in (None, rows):
        logits = emb.torch_project(xt, ct)
        lse = torch.logsumexp(logits, 1, keepdim=True)
        scale = float(max(logits.abs().max(), lse.abs().max()))
        worst = 0.0
        for k in KS:
            ref = torch.topk(logits, k, dim=1)
            values, indices = emb.torch_topk(xt, k, ct)
            assert values.is_cuda and values.dtype == torch.float32 and indices.dtype == torch.int64
            assert values.shape == indices.shape == (130, k) and values.grad_fn is None
            assert torch.equal(values.view(torch.int32), ref.values.view(torch.int32)) and torch.equal(indices, ref.indices), k
            if ct is None:
                equal((values, indices), want, 130, k, ("torch_topk", k))
            lp, li = emb.torch_topk(xt, k, ct, log_probs=True)
            assert torch.equal(li, indices)
            worst = max(worst, float((lp - (ref.values - lse)).abs().max()))
        print("bitlevel %d, %s: log_probs off by at most %.3g = %.3g x the scale %.3g (bound 1e-5 x)"
              % (bitlevel, "all rows" if ct is None else "1025 candidates", worst, worst / scale, scale))
        assert worst <= 1e-5 * scale
    # any shape, dtype and device; x that requires a gradient gives a result without one
    xs = xt[:6].double().reshape(2, 3, dim).cuda().requires_grad_()
    values, indices = emb.torch_topk(xs, 4)
    assert values.shape == indices.shape == (2, 3, 4) and values.grad_fn is None and not values.requires_grad
    equal((values.reshape(6, 4), indices.reshape(6, 4)), want, 6, 4, "any shape")
    with pytest.raises(ValueError):
        emb.torch_topk(xt, 65)
    with pytest.raises(ValueError):
        emb.torch_topk(xt[:, :5], 1)
    emb.close()
    # fewer live candidates than k: index -1 stays -inf with log_probs, the live ones are normalised over the live ones
    packed, table, lists, _, _ = case(dim, bitlevel)
    name, cand, x, want = [e for e in lists if e[0] == "sparse"][0]
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    lp, li = emb.torch_topk(torch.from_numpy(np.array(x)), 33, torch.from_numpy(np.array(cand)), log_probs=True)
    assert np.array_equal(li.cpu().numpy(), want[1][:, :33]) and torch.isneginf(lp[:, 5:]).all()
    assert torch.allclose(torch.exp(lp[:, :5]).sum(1), torch.ones(len(x), device="cuda"), atol=1e-5)
    emb.close()


def test_torch_sample_draws_among_the_k_best(gpu):
    import torch
    dim, bitlevel = 200, 1
    packed, table, lists, big, wide = case(dim, bitlevel)
    name, cand, x, want = wide[0]
    emb = w2b.PackedEmbedding(packed=big, dim=dim, bitlevel=bitlevel)
    xt = torch.from_numpy(np.array(x))
    values, indices = emb.torch_topk(xt, 8)
    greedy = emb.torch_sample(xt, 1)
    assert greedy.dtype == torch.int64 and greedy.shape == (130,) and torch.equal(greedy, indices[:, 0])
    gen = torch.Generator(device="cuda")
    seen = set()
    for seed in (1, 2, 3):
        gen.manual_seed(seed)
        drawn = emb.torch_sample(xt, 8, temperature=4.0, generator=gen)
        assert drawn.shape == (130,) and (drawn[:, None] == indices).any(1).all()
        gen.manual_seed(seed)
        assert torch.equal(emb.torch_sample(xt, 8, temperature=4.0, generator=gen), drawn)       # a fixed generator: the same draw
        seen.add(tuple(drawn.tolist()))
    assert len(seen) == 3 and any((torch.tensor(s, device="cuda") != indices[:, 0]).any() for s in seen)
    assert emb.torch_sample(xt[:6].reshape(2, 3, dim), 8, generator=gen).shape == (2, 3)
    with pytest.raises(ValueError):
        emb.torch_sample(xt, 8, temperature=0.0)
    emb.close()


def test_timing_counts_the_launches_and_the_stated_bytes(gpu):
    rng = np.random.default_rng(67)
    dim, bitlevel, n, m, k = 65, 2, 33, 300, 5
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    cand = topk_cands(rng, ROWS, m)
    x = x_gauss(rng, n, dim)
    wpr = packed.shape[1]
    emb.timing()
    device_form(emb, x, cand, k)
    ms, launches, nbytes = emb.timing()
    assert launches == 1 and ms > 0 and nbytes == 2 * (n * dim * 4 + m * wpr * 8 + m * 8) + n * k * 12
    device_form(emb, x, None, k)
    assert emb.timing()[1:] == (1, 2 * (n * dim * 4 + ROWS * wpr * 8) + n * k * 12)
    emb.topk_device(0, 5, 1)                                                # n == 0: nothing launched
    emb.synchronize()
    assert emb.timing() == (0.0, 0, 0.0)
    emb.close()
