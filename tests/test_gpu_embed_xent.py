"""The packed embedding's softmax cross-entropy on the GPU (include/word2bits_embed.h, "Cross-entropy"): the host form, the
device form by hand and the torch front against the host twin of tests/test_embed_xent_host.py (which ties it to the
definition), bit for bit for mx, se, tl and dx; the chunked gradient path; what the device form does with bad inputs;
the autograd hook; the other buffers of the handle.  The only tolerance is the derived bound of the host test, where
torch's own cross_entropy is the witness."""
import functools

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from test_embed_host import make_table
from test_embed_project_host import host_project, wide_values
from test_embed_backproject_host import host_backproject
from test_embed_xent_host import bounds, host_xent, mild_values, targets_for
from test_gpu_embed import same
from test_gpu_embed_backproject import cand_list

pytestmark = pytest.mark.gpu
ROWS = 300
DIMS = [1, 33, 64, 65, 200, 513]
NS = [1, 33, 65]
MS = [1, 2, 255, 256, 257, 1025, 2500]
SCRATCH = "W2B_EMBED_XENT_SCRATCH"      # the library's override of the bytes of g per gradient launch


def x_sets(rng, table, n):
    """three kinds of vectors: the whole allowed range (logits 2^80 apart: nearly every term is the exact zero), mild ones
    (ordinary probabilities, every g non-zero), and steep ones, 64 x a row of the table: that row's logit stands out by
    64 dim v^2 (1422 at dim 200, one bit), the others stay within a few times 64 sqrt(dim) v^2, so from dim 64 on the
    segments without that row lie more than 64 below the maximum and their U_s is scaled to nothing"""
    dim = table.shape[1]
    return [wide_values(rng, (n, dim)), mild_values(rng, (n, dim)),
            (table[rng.integers(0, len(table), n)] * np.float32(64)).astype(np.float32)]


def twin(packed, dim, bitlevel, x, cand, target):
    rc, mx, se, tl, dx = host_xent(packed, dim, bitlevel, x, cand, target)
    assert rc == 0, _lib.lib().w2b_last_error()
    return mx, se, tl, dx


@functools.lru_cache(maxsize=None)
def case(dim, bitlevel):
    """per (dim, bitlevel): a 300-row and a 2100-row table, and per candidate list (every m of MS, None = all rows of
    either table) three sets of 65 vectors with targets and the twin's results; every n takes the first n, unchanged"""
    rng = np.random.default_rng(19 * dim + bitlevel)
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    big, bigtable = make_table(rng, 2100, dim, bitlevel)
    n = max(NS)
    lists = []
    for m in MS + [None]:
        cand = None if m is None else cand_list(rng, ROWS, m)
        for x in x_sets(rng, table, n):
            target = targets_for(rng, cand, ROWS if m is None else m, n)
            lists.append((cand, x, target, twin(packed, dim, bitlevel, x, cand, target)))
    wide = []
    for x in x_sets(rng, bigtable, n):
        target = targets_for(rng, None, 2100, n)
        wide.append((None, x, target, twin(big, dim, bitlevel, x, None, target)))
    for entry in lists + wide:
        for a in [entry[0], entry[1], entry[2], *entry[3]]:
            if a is not None:
                a.setflags(write=False)
    return packed, lists, big, wide


def host_form(emb, x, cand, target, grad=True):
    """w2b_embed_xent through ctypes: (mx, se, tl, dx), NaN-filled before the call"""
    n = len(x)
    x, target = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(target, np.int32)
    cand = None if cand is None else np.ascontiguousarray(cand, np.int32)
    out = [np.full(n, np.nan, np.float32) for _ in range(3)]
    dx = np.full((n, emb.dim), np.nan, np.float32)
    _lib.check(emb._L.w2b_embed_xent(emb._h, n, x.ctypes.data_as(_lib.f32p), emb.rows if cand is None else cand.size,
                                     None if cand is None else cand.ctypes.data_as(_lib.i32p), target.ctypes.data_as(_lib.i32p),
                                     *[o.ctypes.data_as(_lib.f32p) for o in out], dx.ctypes.data_as(_lib.f32p) if grad else None))
    return (*out, dx)


def device_form(emb, x, cand, target, want_dx=True, slack=0):
    """the device form by hand: reserve, fill the staging views, launch, synchronise, read: (mx, se, tl, dx) as tensors"""
    import torch
    n, m = len(x), emb.rows if cand is None else len(cand)
    x_t, cand_t, tgt_t, stats, dx = emb.staging_xent(n + slack, m + slack)
    assert x_t.shape == (n + slack, emb.dim) and cand_t.dtype == torch.int64 and tgt_t.dtype == torch.int64
    assert stats.shape == (3 * (n + slack),) and dx.shape == (n + slack, emb.dim) and dx.is_cuda
    x_t[:n].copy_(torch.tensor(np.asarray(x, np.float32)))
    tgt_t[:n].copy_(torch.tensor(np.asarray(target, np.int64)))
    if cand is not None:
        cand_t[:m].copy_(torch.tensor(np.asarray(cand, np.int64)))
    stats.fill_(float("nan"))
    dx.fill_(float("nan"))
    torch.cuda.synchronize()
    emb.xent_device(n, m, cand is not None, want_dx)
    emb.synchronize()
    mx, se, tl = stats[:3 * n].view(3, n).clone()
    return mx, se, tl, dx[:n].clone()


def equal(got, want, tag, dx=True):
    for k, name in enumerate(("mx", "se", "tl", "dx")[:4 if dx else 3]):
        assert same(got[k], want[k], "float32"), (tag, name)


def all_forms(emb, x, cand, target, want, tag):
    import torch
    equal(host_form(emb, x, cand, target), want, (tag, "host form"))
    equal(device_form(emb, x, cand, target), want, (tag, "device form"))
    # the torch front: float32 (mx - tl) + log(se) with torch's log on the device, 0 for an ignored vector
    mx, se, tl = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in want[:3])
    live = torch.from_numpy(target >= 0).cuda()
    loss = torch.where(live, (mx - tl) + torch.log(torch.where(live, se, torch.ones_like(se))), torch.zeros_like(se))
    got = emb.torch_xent(torch.from_numpy(x), torch.from_numpy(target), None if cand is None else torch.from_numpy(cand))
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (len(x),)
    assert torch.equal(got.view(torch.int32), loss.view(torch.int32)), (tag, "torch")


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", DIMS)
def test_every_form_equals_the_twin(gpu, dim, bitlevel):
    """every n x every candidate list x the three kinds of x, in the three forms; then all 2100 rows of a second table
    (nine segments, the last partial)"""
    packed, lists, big, wide = case(dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    for k, (cand, x, target, want) in enumerate(lists):
        for n in NS:
            all_forms(emb, np.ascontiguousarray(x[:n]), cand, target[:n], [a[:n] for a in want],
                      (n, None if cand is None else len(cand), k % 3))
    assert emb.bad_ids() == 0
    # the numpy front: float64 loss from the same three numbers, any shape
    cand, x, target, want = lists[3 * 4 + 1]
    loss, dx = emb.xent(x[:6].reshape(2, 3, dim), target[:6].reshape(2, 3), cand, grad=True)
    mx, se, tl = (a[:6].astype(np.float64) for a in want[:3])
    ref = np.where(target[:6] >= 0, (mx - tl) + np.log(se), 0.0)
    assert loss.dtype == np.float64 and loss.shape == (2, 3) and np.array_equal(loss.reshape(6), ref)
    assert same(dx.reshape(6, dim), want[3][:6], "float32") and emb.xent(x[:6], target[:6], cand).shape == (6,)
    emb.close()
    emb = w2b.PackedEmbedding(packed=big, dim=dim, bitlevel=bitlevel)
    for k, (cand, x, target, want) in enumerate(wide):
        for n in (1, 65):
            all_forms(emb, np.ascontiguousarray(x[:n]), None, target[:n], [a[:n] for a in want], (n, "2100 rows", k))
    emb.close()


def test_the_kinds_of_x_reach_the_branches_they_are_meant_for():
    """in the twin alone (no device), at m = 2500 from 300 rows: every steep vector has a segment whose maximum lies more
    than 64 below mx (a segment of 256 draws misses the vector's own row with probability 0.43), the mild ones have none
    and no zero term at all, the wide ones hardly anything but zero terms"""
    packed, lists, _, _ = case(200, 1)
    seen = {}
    for k, (cand, x, target, want) in enumerate(lists):
        if cand is None or len(cand) != 2500:
            continue
        rc, l = host_project(packed, 200, 1, x, cand)
        assert rc == 0
        live = cand >= 0
        below = np.zeros(len(x), int)
        for j0 in range(0, 2500, 256):
            seg = l[:, j0:j0 + 256][:, live[j0:j0 + 256]]
            below += (seg.max(axis=1) < want[0] - 64)
        seen[k % 3] = (below, (l[:, live] < (want[0] - 64)[:, None]).mean())
    assert (seen[2][0] >= 1).all() and (seen[1][0] == 0).all() and seen[1][1] == 0 and seen[0][1] > 0.9


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_the_chunked_gradient_gives_the_same_bits(gpu, monkeypatch, bitlevel):
    """The gradient goes through a scratch of at most 64 MiB of g: whole vectors that fit, or, when one vector's m candidates
    do not, one vector x candidate ranges of a multiple of W2B_EMBED_WSEG positions, S carried by the back-projection.
    Neither switch can be crossed at a shape a test can afford, so W2B_EMBED_XENT_SCRATCH lowers the 64 MiB: 8192 bytes at
    m = 257 are 7 vectors a launch (65 vectors: 10 launches, windows that begin inside a pair of vector tiles), 4096 bytes
    at m = 2500 are 1024 candidates a launch.  Each against the unchunked call and against the twin."""
    dim = 200
    packed, lists, _, _ = case(dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    for cand, x, target, want in lists:
        if cand is None or len(cand) not in (257, 2500):
            continue
        monkeypatch.delenv(SCRATCH, raising=False)
        emb.timing()
        whole = device_form(emb, x, cand, target)
        assert emb.timing()[1] == 2                                          # statistics, one gradient chunk
        monkeypatch.setenv(SCRATCH, "8192" if len(cand) == 257 else "4096")
        chunked = device_form(emb, x, cand, target)
        assert emb.timing()[1] == (1 + 10 if len(cand) == 257 else 1 + 65 * 3)
        equal(chunked, [a.cpu().numpy() for a in whole], len(cand))
        equal(chunked, want, len(cand))
        equal(host_form(emb, x, cand, target), want, (len(cand), "host form, chunked"))
    emb.close()


def test_want_dx_0_leaves_dx_untouched_and_reserve_keeps_its_pointers(gpu):
    import torch
    rng = np.random.default_rng(31)
    dim, bitlevel = 65, 2
    packed, lists, _, _ = case(dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    cand, x, target, want = lists[3 * 5 + 1]                                  # m = 1025, mild
    mx, se, tl, dx = device_form(emb, x, cand, target, want_dx=False)
    equal((mx, se, tl), want, "statistics only", dx=False)
    assert torch.isnan(dx).all()
    got = emb.torch_xent(torch.from_numpy(x), torch.from_numpy(target), torch.from_numpy(cand), reduction="sum")
    assert got.shape == () and got.grad_fn is None
    # buffers of its own: growing the others leaves them, growing them leaves the others
    others = (emb.reserve(50, 2), emb.reserve_weights(50), emb.reserve_project(4, 10), emb.reserve_backproject(4, 10))
    small = emb.reserve_xent(65, 1025)
    assert emb.reserve_xent(2, 5) == small and len(small) == 5 and len(set(small)) == 5
    grown = emb.reserve_xent(65, 2000)                                       # more candidates: only cand_dev may move
    assert (grown[0], grown[2], grown[3], grown[4]) == (small[0], small[2], small[3], small[4])
    assert (emb.reserve(50, 2), emb.reserve_weights(50), emb.reserve_project(4, 10), emb.reserve_backproject(4, 10)) == others
    emb.reserve(5000, 100)
    emb.reserve_project(50, 400)
    emb.reserve_backproject(40, 400)
    assert emb.reserve_xent(65, 2000) == grown
    for args in ((66, 5), (5, 2001), (-1, 5), (5, -1)):
        with pytest.raises(w2b.W2bError) as e:
            emb.xent_device(*args)
        assert e.value.code == _lib.W2B_EINVAL, args
    with pytest.raises(w2b.W2bError) as e:
        emb.xent_device(5, 2000, False)                                      # all rows: m must be rows
    assert e.value.code == _lib.W2B_EINVAL
    fresh = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    with pytest.raises(w2b.W2bError):
        fresh.xent_device(1, 1)                                              # nothing reserved
    fresh.close()
    emb.close()


def test_device_form_ignores_and_counts_what_is_out_of_range(gpu):
    """targets >= m and on padding, candidates >= rows and a target on one of them, written into the staging (reserved a
    little larger, so that even an unclamped access would stay inside the allocations): the stated effect and count"""
    import torch
    rng = np.random.default_rng(37)
    dim, bitlevel, n, m = 200, 2, 70, 1500
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    cand = rng.integers(0, ROWS, m).astype(np.int64)
    cand[[3, 77]] = -1, -9
    bad = [17, 64, 1400, 1499]
    plant = cand.copy()
    plant[bad] = ROWS, ROWS + 5, 1 << 40, 2 ** 31
    clean = cand.copy()
    clean[bad] = -1
    x = mild_values(rng, (n, dim))
    target = targets_for(rng, clean.astype(np.int32), m, n).astype(np.int64)
    planted = target.copy()
    planted[[5, 6, 7, 8, 9]] = m, 1 << 40, 3, 64, m + 63                     # >= m, far beyond, on padding, on a refused candidate
    effective = target.copy()
    effective[[5, 6, 7, 8, 9]] = -1
    want = twin(packed, dim, bitlevel, x, clean.astype(np.int32), effective.astype(np.int32))
    got = device_form(emb, x, plant, planted, slack=64)
    equal(got, want, "bad inputs")
    assert emb.bad_ids() == len(bad) + 5 and emb.bad_ids() == 0
    assert not got[3][5:10].view(torch.int32).any() and not got[2][5:10].view(torch.int32).any()
    with pytest.raises(w2b.W2bError) as e:
        emb.torch_xent(torch.from_numpy(x), torch.from_numpy(planted), torch.from_numpy(plant))
    assert e.value.code == _lib.W2B_EINVAL and emb.bad_ids() == 0
    emb.timing()
    for c, t in ((np.array([1, ROWS], np.int32), [0]), (np.array([1, -1], np.int32), [1]), (np.array([1, 2], np.int32), [2])):
        with pytest.raises(w2b.W2bError) as e:                              # the host form refuses each before any launch
            emb.xent(x[:1], np.array(t, np.int32), c)
        assert e.value.code == _lib.W2B_EINVAL
    with pytest.raises(w2b.W2bError) as e:
        emb.xent(np.full((1, dim), np.inf, np.float32), np.zeros(1, np.int32))
    assert e.value.code == _lib.W2B_EINVAL and emb.timing()[1] == 0
    # nothing live, and m == 0: mx = se = tl = +0.0, dx = +0.0, no target is acceptable
    pad = np.full(300, -1, np.int64)
    for c in (pad, pad[:0]):
        got = device_form(emb, x[:5], c, np.array([-1, 0, -1, 7, -1]))
        assert not any(a.view(torch.int32).any() for a in got) and emb.bad_ids() == 2
    emb.close()


def test_autograd_gives_the_twins_gradient(gpu):
    import torch
    import torch.nn.functional as F
    dim, bitlevel = 200, 2
    packed, lists, _, _ = case(dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    for k in (3 * 6 + 1, 3 * 7 + 1):                                         # m = 2500 and all rows, mild x
        cand, x, target, want = lists[k]
        ct = None if cand is None else torch.from_numpy(cand)
        count = int((target >= 0).sum())
        xt = torch.from_numpy(x).cuda().requires_grad_()
        loss = emb.torch_xent(xt, torch.from_numpy(target), ct, reduction="mean")
        assert loss.grad_fn is not None and loss.shape == () and loss.is_cuda
        loss.backward()
        # backward multiplies dx by the incoming gradient, which is 1 / count from the mean's division
        scale = (torch.ones((), device="cuda") / torch.tensor(float(count), device="cuda"))
        ref = torch.from_numpy(np.ascontiguousarray(want[3])).cuda() * scale
        assert torch.equal(xt.grad.view(torch.int32), ref.view(torch.int32))
        # "none" with a gradient per vector, float64 x on the CPU and any shape: dx * grad_out, in x's dtype and device
        xc = torch.from_numpy(x[:6]).double().reshape(2, 3, dim).requires_grad_()
        G = torch.tensor([[1.0, 2.0, -0.5], [0.25, 4.0, 0.0]], dtype=torch.float64)
        emb.torch_xent(xc, torch.from_numpy(target[:6]).reshape(2, 3), ct).backward(G.cuda().float())
        ref = torch.from_numpy(np.ascontiguousarray(want[3][:6])) * G.reshape(6, 1).float()
        assert xc.grad.dtype == torch.float64 and xc.grad.shape == (2, 3, dim) and not xc.grad.is_cuda
        assert torch.equal(xc.grad.reshape(6, dim).float().view(torch.int32), ref.view(torch.int32))
        # torch's own cross_entropy on the logits of torch_project, within the derived bound of the host test
        xr = torch.from_numpy(x).cuda().requires_grad_()
        logits = emb.torch_project(xr, ct)
        if cand is not None:
            logits = logits.masked_fill(torch.from_numpy(cand < 0).cuda(), float("-inf"))
        tt = torch.from_numpy(target).long().cuda()
        ref_loss = F.cross_entropy(logits.double(), tt, ignore_index=-1, reduction="mean")
        ref_loss.backward()
        mm = ROWS if cand is None else len(cand)
        lmax = float(logits.detach()[torch.isfinite(logits.detach())].abs().max())
        b_loss, b_dx = bounds(mm, bitlevel, lmax)
        # On top of the host test's bounds, which are against an exact reference, what float32 adds on either side here.
        # Loss: (mx - tl) + log(se) rounds three times more (each below 2 lmax + log m), the mean once per vector and once
        # for the division.  Gradient: the witness rounds its g to float32 (u of sum |g| <= 2) and sends it through the
        # same back-projection chains (the chain term of bounds() once more), and both sides round the product with
        # 1 / count twice (2 u of |dx| <= 2 vmax, vmax = 0.75).
        u = 2.0 ** -24
        f32_loss = u * (3 * (2 * lmax + np.log(mm)) + (len(x) + 1) * float(ref_loss))
        f32_dx = 0.75 * (2 * u + 2 * (min(mm, 1024) + -(-mm // 1024) + 1) * u) + 2 * (2 * u * 2 * 0.75)
        e_loss = abs(float(loss) - float(ref_loss))
        e_dx = float((xt.grad.double() - xr.grad.double()).abs().max()) * count
        print("m = %d: loss off by %.3g (bound %.3g), dx off by %.3g (bound %.3g)" % (mm, e_loss, b_loss + f32_loss, e_dx, b_dx + f32_dx))
        assert e_loss <= b_loss + f32_loss and e_dx <= b_dx + f32_dx
    # no gradient asked for: nothing is recorded, and no dx is computed
    cand, x, target, want = lists[3 * 6 + 1]
    emb.timing()
    assert emb.torch_xent(torch.from_numpy(x).cuda(), torch.from_numpy(target), torch.from_numpy(cand)).grad_fn is None
    with torch.no_grad():
        assert emb.torch_xent(torch.from_numpy(x).cuda().requires_grad_(), torch.from_numpy(target), torch.from_numpy(cand)).grad_fn is None
    assert emb.timing()[1] == 2
    with pytest.raises(ValueError):
        emb.torch_xent(torch.from_numpy(x), torch.from_numpy(target), reduction="max")
    with pytest.raises(ValueError):
        emb.torch_xent(torch.from_numpy(x), torch.from_numpy(target[:5]))
    emb.close()


def test_the_other_calls_on_the_handle_are_not_disturbed(gpu):
    """torch_project, torch_backproject and torch_bag before and after a cross-entropy call with its gradient: their twins'
    results both times"""
    import torch
    from test_embed_host import ref_bag
    rng = np.random.default_rng(41)
    dim, bitlevel, m = 65, 1, 700
    packed, table = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    cand = cand_list(rng, ROWS, m)
    x = wide_values(rng, (33, dim))
    g = wide_values(rng, (33, m))
    ids = rng.integers(0, ROWS, 90).astype(np.int32)
    offsets = np.array([0, 10, 10, 90], np.int64)
    rc, want_p = host_project(packed, dim, bitlevel, x, cand)
    rc2, want_b = host_backproject(packed, dim, bitlevel, g, cand)
    assert rc == 0 and rc2 == 0
    want_bag = ref_bag(table, bitlevel, ids, offsets, "sum")
    target = targets_for(rng, cand, m, 33)
    want = twin(packed, dim, bitlevel, x, cand, target)

    def others():
        ct = torch.from_numpy(cand)
        assert same(emb.torch_project(torch.from_numpy(x), ct), want_p, "float32")
        assert same(emb.torch_backproject(torch.from_numpy(g), ct), want_b, "float32")
        assert same(emb.torch_bag(torch.from_numpy(ids), torch.from_numpy(offsets), "sum"), want_bag, "float32")

    others()
    views = (emb.torch_project(torch.from_numpy(x), torch.from_numpy(cand), copy=False),
             emb.torch_backproject(torch.from_numpy(g), torch.from_numpy(cand), copy=False))
    equal(device_form(emb, x, cand, target), want, "between")
    assert same(views[0], want_p, "float32") and same(views[1], want_b, "float32")       # the views of their buffers still hold
    others()
    emb.close()


def test_timing_counts_the_launches_and_the_stated_bytes(gpu):
    rng = np.random.default_rng(47)
    dim, bitlevel, n, m = 65, 2, 33, 300
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    cand = cand_list(rng, ROWS, m)
    x = mild_values(rng, (n, dim))
    target = targets_for(rng, cand, m, n)
    wpr = packed.shape[1]
    stats_bytes = n * dim * 4 + m * wpr * 8 + m * 8 + n * 8 + n * 12
    emb.timing()
    device_form(emb, x, cand, target, want_dx=False)
    ms, launches, nbytes = emb.timing()
    assert launches == 1 and ms > 0 and nbytes == stats_bytes
    device_form(emb, x, cand, target)
    ms, launches, nbytes = emb.timing()
    assert launches == 2 and nbytes == stats_bytes + 2 * (m * wpr * 8 + m * 8) + 2 * n * m * 4 + 2 * n * dim * 4
    device_form(emb, x, None, targets_for(rng, None, ROWS, n))
    assert emb.timing()[2] == (stats_bytes - m * 8) + 2 * (m * wpr * 8) + 2 * n * m * 4 + 2 * n * dim * 4
    emb.xent_device(0, 5)                                                   # n == 0: nothing launched
    emb.synchronize()
    assert emb.xent(np.zeros((0, dim), np.float32), np.zeros(0, np.int32)).shape == (0,)
    assert emb.timing() == (0.0, 0, 0.0)
    emb.close()
