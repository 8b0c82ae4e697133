"""The packed embedding's back-projection on the GPU (include/word2bits_embed.h, "Back-projection"): the host form, the
device form and the torch front against the host twin of tests/test_embed_backproject_host.py (which ties it to the
definition of the weighted bag), bit for bit; both paths of the driver; the weighted bag on the same handle; torch as an
independent witness; the autograd hook of torch_project.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from test_embed_host import host_lookup, make_table
from test_embed_backproject_host import host_backproject
from test_embed_project_host import wide_values
from test_gpu_embed import same

pytestmark = pytest.mark.gpu
ROWS = 300
DIMS = [1, 3, 31, 32, 33, 64, 65, 200, 513, 800]
NS = [1, 31, 32, 33, 65, 130]
MS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2500]
PATH = "W2B_EMBED_BACK_PATH"       # the library's override of the driver's choice: "registers" / "scratch"


def cand_list(rng, rows, m):
    """m candidates with repeats; padding at the first, a middle and the last position (m >= 14)"""
    cand = rng.integers(0, rows, m).astype(np.int32)
    if m >= 14:
        cand[[5, 6, m - 2]] = cand[2], cand[2], rows - 1
        cand[[0, m // 2, m - 1]] = -1, -3, -1
    return cand


def planted(rng, n, cand, m=None):
    """g over the whole allowed range, NaN at the padding positions"""
    g = wide_values(rng, (n, len(cand) if m is None else m))
    if cand is not None:
        g[:, cand < 0] = np.nan
    return g


def twin(packed, dim, bitlevel, g, cand):
    rc, want = host_backproject(packed, dim, bitlevel, g, cand)
    assert rc == 0
    return want


@functools.lru_cache(maxsize=None)
def case(dim, bitlevel):
    """per (dim, bitlevel): a 300-row and a 2100-row table, and per candidate list (every m of MS, and None = all rows of
    either table) 130 vectors of g with the twin's result; every n below takes the first n vectors of it, unchanged"""
    rng = np.random.default_rng(17 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    big, _ = make_table(rng, 2100, dim, bitlevel)
    lists = []
    for m in MS:
        cand = cand_list(rng, ROWS, m)
        g = planted(rng, max(NS), cand)
        lists.append((cand, g, twin(packed, dim, bitlevel, g, cand)))
    g = wide_values(rng, (max(NS), ROWS))
    lists.append((None, g, twin(packed, dim, bitlevel, g, None)))
    g = wide_values(rng, (max(NS), 2100))
    wide = (g, twin(big, dim, bitlevel, g, None))
    for a in [packed, big, *wide] + [x for l in lists for x in l if x is not None]:
        a.setflags(write=False)
    return packed, lists, big, wide


def device_backproject(emb, g, cand, slack=0):
    """the device form by hand: reserve, fill the staging views, launch, synchronise, read"""
    import torch
    n, m = g.shape
    g_t, cand_t, dx = emb.staging_backproject(n + slack, m + slack)
    assert g_t.dtype == torch.float32 and g_t.shape == ((n + slack) * (m + slack),) and cand_t.dtype == torch.int64
    assert dx.dtype == torch.float32 and dx.shape == (n + slack, emb.dim) and dx.is_cuda
    g_t[:n * m].copy_(torch.tensor(np.asarray(g, np.float32)).reshape(-1))      # (a copy: the cached g is read-only)
    if cand is not None:
        cand_t[:m].copy_(torch.from_numpy(np.asarray(cand, np.int64)))
    dx.fill_(float("nan"))
    torch.cuda.synchronize()
    emb.backproject_device(n, m, cand is not None)
    emb.synchronize()
    return dx[:n].clone()


def all_forms(emb, g, cand, want, tag):
    import torch
    got = emb.backproject(g, cand)
    assert got.dtype == np.float32 and same(got, want, "float32"), (tag, "host form")
    assert same(device_backproject(emb, g, cand), want, "float32"), (tag, "device form")
    got = emb.torch_backproject(torch.tensor(g), None if cand is None else torch.tensor(cand))
    assert got.is_cuda and got.dtype == torch.float32 and same(got, want, "float32"), (tag, "torch")


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", DIMS)
def test_every_form_equals_the_twin(gpu, dim, bitlevel):
    """every n x every candidate list of the parametrisation, in the three forms"""
    import torch
    packed, lists, big, (gbig, wbig) = case(dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    for cand, g, want in lists:
        for n in NS:
            all_forms(emb, np.ascontiguousarray(g[:n]), cand, want[:n], (n, None if cand is None else len(cand)))
    cand, g, want = lists[-2]                                                  # any shape, any float and integer type
    got = emb.torch_backproject(torch.tensor(np.nan_to_num(g[:6])).reshape(2, 3, -1).cuda().double(),
                                torch.tensor(cand).cuda().int())
    assert got.shape == (2, 3, dim) and same(got.reshape(6, dim), want[:6], "float32")
    assert emb.backproject(np.nan_to_num(g[:6]).reshape(3, 2, -1), cand).shape == (3, 2, dim)
    emb.close()
    emb = w2b.PackedEmbedding(packed=big, dim=dim, bitlevel=bitlevel)          # all 2100 rows: three segments, the last partial
    for n in (1, 33, 130):
        all_forms(emb, np.ascontiguousarray(gbig[:n]), None, wbig[:n], (n, "2100 rows"))
    emb.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_both_paths_of_the_driver_give_the_twins_bits(gpu, monkeypatch, bitlevel):
    """The driver keeps S in registers when vector tiles x column tiles fill the device and sends the segments through the
    scratch and the finishing kernel otherwise.  The switch (256 tiles of 128 x 128) cannot be crossed at shapes a test
    can afford, so the library's override W2B_EMBED_BACK_PATH forces either path here, at n = 130 / dim 800 and n = 1 /
    dim 33 with m = 2500, and without it the driver's own choice runs.  n = 2 / dim 800 against 150 000 candidates is more
    segments than one launch of the scratch path takes (146 at 7 tiles): ranges of segments, S carried by the finishing step."""
    rng = np.random.default_rng(61 + bitlevel)
    for n, dim, m in ((130, 800, 2500), (1, 33, 2500), (2, 800, 150_000)):
        packed, _ = make_table(rng, ROWS, dim, bitlevel)
        emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
        cand = cand_list(rng, ROWS, m)
        g = planted(rng, n, cand)
        want = twin(packed, dim, bitlevel, g, cand)
        for path in ("registers", "scratch", None):
            if path is None:
                monkeypatch.delenv(PATH, raising=False)
            else:
                monkeypatch.setenv(PATH, path)
            assert same(device_backproject(emb, g, cand), want, "float32"), (n, dim, m, path, "device form")
            assert same(emb.backproject(g, cand), want, "float32"), (n, dim, m, path, "host form")
        emb.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [65, 200])
def test_it_equals_the_weighted_bag_on_the_same_handle(gpu, dim, bitlevel):
    import torch
    rng = np.random.default_rng(7 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    n, m = 33, 2500
    cand = cand_list(rng, ROWS, m)
    g = wide_values(rng, (n, m))
    want = emb.bag(np.tile(cand, n), np.arange(n + 1, dtype=np.int64) * m, "sum", per_sample_weights=g.reshape(-1))
    assert same(emb.backproject(g, cand), want, "float32")
    got = emb.torch_backproject(torch.from_numpy(g), torch.from_numpy(cand))
    tb = emb.torch_bag(torch.from_numpy(np.tile(cand, n)), torch.arange(n + 1) * m, "sum",
                       per_sample_weights=torch.from_numpy(g.reshape(-1)))
    assert torch.equal(got.view(torch.int32), tb.view(torch.int32))
    eye = np.eye(m, dtype=np.float32)[:130]                                 # consequence (b): one-hot reads the table
    assert same(emb.backproject(eye, cand), host_lookup(packed, dim, bitlevel, cand[:130])[1], "float32")
    emb.close()


def test_torch_is_an_independent_witness_at_two_bits(gpu):
    """|g| <= 8 integers, m = 2500, dim 200: every partial sum is an integer below 2^24 and the order is irrelevant, so
    torch's float64 g @ codes[cand], times 0.25, on the expanded table is the float32 output exactly"""
    import torch
    rng = np.random.default_rng(37)
    dim, m = 200, 2500
    packed, table = make_table(rng, ROWS, dim, 2)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=2)
    cand = cand_list(rng, ROWS, m)
    g = rng.integers(-8, 9, (130, m)).astype(np.float32)
    codes = torch.from_numpy(table).double().cuda() * 4.0                   # +-1 / +-3, exact
    masked = torch.from_numpy(np.where(cand < 0, 0.0, g)).double().cuda()   # padding columns out of g
    want = ((masked @ codes[torch.from_numpy(np.maximum(cand, 0)).long().cuda()]) * 0.25).float()
    got = emb.torch_backproject(torch.from_numpy(g), torch.from_numpy(cand))
    assert torch.equal(got.view(torch.int32), (want + 0.0).view(torch.int32))
    g = rng.integers(-8, 9, (65, ROWS)).astype(np.float32)
    want = ((torch.from_numpy(g).double().cuda() @ codes) * 0.25).float()
    assert torch.equal(emb.torch_backproject(torch.from_numpy(g)).view(torch.int32), (want + 0.0).view(torch.int32))
    emb.close()


def test_torch_project_is_differentiable_with_respect_to_x(gpu):
    import torch
    rng = np.random.default_rng(43)
    dim, m = 65, 301
    packed, table = make_table(rng, ROWS, dim, 2)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=2)
    cand = torch.from_numpy(cand_list(rng, ROWS, m))
    for c, width in ((cand, m), (None, ROWS)):
        G = torch.from_numpy(wide_values(rng, (6, width))).cuda()
        for x in (torch.from_numpy(wide_values(rng, (6, dim))).cuda(),
                  torch.from_numpy(wide_values(rng, (2, 3, dim))).double()):    # float64 on the CPU, any shape
            x.requires_grad_()
            y = emb.torch_project(x, c)
            assert y.grad_fn is not None and y.is_cuda and y.shape == tuple(x.shape[:-1]) + (width,)
            assert torch.equal(y.detach().view(torch.int32), emb.torch_project(x.detach(), c).view(torch.int32))
            y.backward(G.reshape(y.shape))
            want = emb.torch_backproject(G, c)
            assert x.grad.dtype == x.dtype and x.grad.shape == x.shape and x.grad.device == x.device
            assert torch.equal(x.grad.reshape(6, dim).float().cpu().view(torch.int32), want.cpu().view(torch.int32))
    # 16-bit logits: the backward receives bf16 and back-projects it cast to float32
    x = torch.from_numpy(wide_values(rng, (6, dim))).cuda().requires_grad_()
    y = emb.torch_project(x, cand, dtype=torch.bfloat16)
    assert y.dtype == torch.bfloat16 and y.grad_fn is not None
    G = torch.from_numpy(rng.integers(-64, 65, (6, m)).astype(np.float32)).cuda().bfloat16()
    y.backward(G)
    assert torch.equal(x.grad.view(torch.int32), emb.torch_backproject(G.float(), cand).view(torch.int32))
    # the integer regime: torch's own autograd through x @ W[cand].T on the float table gives the same gradient exactly
    xi = torch.from_numpy(rng.integers(-8, 9, (6, dim)).astype(np.float32)).cuda()
    Gi = torch.from_numpy(rng.integers(-8, 9, (6, m)).astype(np.float32)).cuda()
    W = torch.from_numpy(table).cuda()
    live = (cand >= 0).cuda()
    a = xi.clone().requires_grad_()
    emb.torch_project(a, cand).backward(Gi)
    b = xi.clone().requires_grad_()
    ((b @ W[cand.clamp(min=0).cuda()].T) * live).backward(Gi)
    assert torch.equal(a.grad.view(torch.int32), (b.grad + 0.0).view(torch.int32)) and a.grad.abs().max() > 0
    # no gradient asked for: nothing changes
    x = torch.from_numpy(wide_values(rng, (6, dim))).cuda()
    assert emb.torch_project(x, cand).grad_fn is None
    with torch.no_grad():
        assert emb.torch_project(x.clone().requires_grad_(), cand).grad_fn is None
    view = emb.torch_project(x, cand, copy=False)
    assert view.grad_fn is None and view.data_ptr() == emb.reserve_project(6, m)[2]
    emb.close()


def test_a_large_call_is_chunked_and_keeps_its_bits(gpu, monkeypatch):
    """n = 70 vectors against all of 300 000 rows at dim 64: 84 MB of g, more than one 64 MiB chunk of the host form, cut
    between two candidate ranges with S carried across.  Vectors 0, 69 and three random ones against the twin (the others
    are not computed on the host).  One tile: the driver sends the segments through the scratch; the override repeats the
    call with S in registers."""
    rng = np.random.default_rng(15)
    rows, dim, bitlevel, n = 300_000, 64, 2, 70
    packed = rng.integers(0, 2 ** 64, (rows, 2), dtype=np.uint64)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    g = wide_values(rng, (n, rows))
    emb.timing()
    got = emb.backproject(g)
    assert got.shape == (n, dim) and g.nbytes > (64 << 20) and emb.timing()[1] >= 2
    monkeypatch.setenv(PATH, "registers")
    assert same(emb.backproject(g), got, "float32")
    for i in [0, n - 1] + rng.integers(1, n - 1, 3).tolist():
        assert same(got[i:i + 1], twin(packed, dim, bitlevel, g[i:i + 1], None), "float32"), i
    emb.close()


def test_device_form_ignores_and_counts_what_is_out_of_range(gpu):
    """candidates >= rows and < 0 written into the staging (reserved a little larger, so that even an unclamped access
    would stay inside the allocations: a missing clamp shows as a wrong result or count), NaN in their columns of g"""
    import torch
    rng = np.random.default_rng(19)
    dim, bitlevel = 200, 2
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    cand = rng.integers(0, ROWS, 1500).astype(np.int64)
    cand[[3, 77]] = -1, -9
    bad = [17, 64, 1400, 1499]
    plant = cand.copy()
    plant[bad] = ROWS, ROWS + 5, 1 << 40, 2 ** 31
    clean = cand.copy()
    clean[bad] = -1
    g = wide_values(rng, (70, 1500))
    g[:, bad + [3, 77]] = np.nan
    want = twin(packed, dim, bitlevel, g, clean.astype(np.int32))
    assert same(device_backproject(emb, g, plant, slack=64), want, "float32")
    assert emb.bad_ids() == len(bad) and emb.bad_ids() == 0
    with pytest.raises(w2b.W2bError) as e:
        emb.torch_backproject(torch.from_numpy(g), torch.from_numpy(plant))
    assert e.value.code == _lib.W2B_EINVAL and emb.bad_ids() == 0
    emb.timing()
    with pytest.raises(w2b.W2bError) as e:                                  # the host form refuses it before any launch
        emb.backproject(np.ones((1, 2), np.float32), np.array([1, ROWS], np.int32))
    assert e.value.code == _lib.W2B_EINVAL
    with pytest.raises(w2b.W2bError) as e:
        emb.backproject(np.full((1, ROWS), np.inf, np.float32))
    assert e.value.code == _lib.W2B_EINVAL and emb.timing()[1] == 0
    emb.close()


def test_reserve_backproject_has_buffers_of_its_own_and_refuses_more_than_it_holds(gpu):
    import torch
    rng = np.random.default_rng(23)
    dim, bitlevel = 65, 1
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    ids = rng.integers(0, ROWS, 50).astype(np.int32)
    ids_t, _, rows_out = emb.staging(50, 2)
    w_ptr = emb.reserve_weights(50)
    base = emb.reserve(50, 2)
    proj = emb.reserve_project(4, 10)
    ids_t.copy_(torch.from_numpy(ids.astype(np.int64)))
    small = emb.reserve_backproject(4, 10)
    assert emb.reserve_backproject(2, 5) == small                           # asking for less changes nothing
    big = emb.reserve_backproject(40, ROWS + 10)                            # growing the back-projection's buffers ...
    assert emb.reserve_backproject(4, 10) == big and emb.reserve_backproject(40, ROWS) == big
    assert emb.reserve(50, 2) == base and emb.reserve_weights(50) == w_ptr and emb.reserve_project(4, 10) == proj   # ... leaves the others
    torch.cuda.synchronize()
    emb.lookup_device(50)
    emb.synchronize()
    assert same(rows_out[:50].clone(), host_lookup(packed, dim, bitlevel, ids)[1], "float32")
    emb.reserve(5000, 100)                                                  # and the other way round
    emb.reserve_weights(5000)
    emb.reserve_project(50, 400)
    assert emb.reserve_backproject(40, ROWS + 10) == big
    g = wide_values(rng, (40, ROWS))
    assert same(device_backproject(emb, g, None), twin(packed, dim, bitlevel, g, None), "float32")
    assert emb.reserve_backproject(40, ROWS + 10) == big
    for args in ((41, ROWS, True), (40, ROWS + 11, True), (40, ROWS + 10, True), (40, ROWS + 10, False), (-1, 5, True),
                 (5, -1, True)):
        if args == (40, ROWS + 10, True):
            emb.backproject_device(*args)                                   # exactly what was reserved is fine
            continue
        with pytest.raises(w2b.W2bError) as e:
            emb.backproject_device(*args)
        assert e.value.code == _lib.W2B_EINVAL, args
    emb.synchronize()
    assert emb.bad_ids() >= 0
    fresh = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    with pytest.raises(w2b.W2bError):
        fresh.backproject_device(1, 1)                                      # nothing reserved
    fresh.reserve_backproject(4, 8)
    with pytest.raises(w2b.W2bError) as e:
        fresh.backproject_device(4, 8, False)                               # all rows need max_m >= rows
    assert e.value.code == _lib.W2B_EINVAL
    with pytest.raises(ValueError):
        fresh.backproject(np.zeros((2, ROWS + 1), np.float32))
    fresh.close()
    emb.close()


def test_timing_counts_the_launches_and_the_stated_bytes(gpu):
    import torch
    rng = np.random.default_rng(29)
    dim, bitlevel = 65, 2
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    cand = cand_list(rng, ROWS, 127)
    g = wide_values(rng, (33, 127))
    wpr = packed.shape[1]
    emb.timing()
    device_backproject(emb, g, cand)
    ms, launches, nbytes = emb.timing()
    assert launches == 1 and ms > 0 and nbytes == 33 * 127 * 4 + 127 * wpr * 8 + 127 * 8 + 33 * dim * 4
    device_backproject(emb, wide_values(rng, (33, ROWS)), None)
    emb.backproject(g, cand)
    ms, launches, nbytes = emb.timing()
    assert launches == 2 and nbytes == (33 * ROWS * 4 + ROWS * wpr * 8 + 33 * dim * 4) + \
        (33 * 127 * 4 + 127 * wpr * 8 + 127 * 8 + 33 * dim * 4)
    emb.backproject_device(0, 5)                                            # n == 0 and m == 0: nothing launched
    emb.backproject_device(5, 0)
    emb.synchronize()
    assert emb.backproject(np.zeros((0, ROWS), np.float32)).shape == (0, dim)
    zero = emb.backproject(np.zeros((33, 0), np.float32), np.zeros(0, np.int32))
    assert zero.shape == (33, dim) and not zero.view(np.uint32).any()       # an empty sum: +0.0 rows
    assert emb.torch_backproject(torch.zeros(0, ROWS)).shape == (0, dim)
    zero = emb.torch_backproject(torch.from_numpy(g[:, :0]), torch.zeros(0, dtype=torch.int64))
    assert zero.shape == (33, dim) and not zero.view(torch.int32).any()
    assert emb.timing() == (0.0, 0, 0.0)
    emb.close()
