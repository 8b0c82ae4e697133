"""The packed embedding's projection on the GPU (include/word2bits_embed.h, "Projection"): the host form, the device form
and the torch front against the host twin of tests/test_embed_project_host.py (which ties it to the numpy definition), bit
for bit; bf16 / f16 against the twin's float32 result rounded to nearest even.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from test_embed_host import host_lookup, make_table
from test_embed_project_host import host_project, wide_values
from test_gpu_embed import DTYPES, ROWS, same, tdtype

pytestmark = pytest.mark.gpu
DIMS = [1, 3, 7, 8, 9, 63, 64, 65, 200, 512, 513, 800, 1089]
NS = [1, 31, 32, 33, 65, 130]
CANDS = [None, 1, 31, 33, 127, 300, 301]


def cand_list(rng, m):
    """m candidate rows; the list of 301 has repeats and padding"""
    if m is None:
        return None
    cand = rng.integers(0, ROWS, m).astype(np.int32)
    if m == 301:
        cand[[0, 64, 299]] = -1, -3, -1
        cand[[5, 6, 300]] = cand[4], cand[4], ROWS - 1
    return cand


def twin(packed, dim, bitlevel, x, cand):
    rc, want = host_project(packed, dim, bitlevel, x, cand)
    assert rc == 0
    return want


@functools.lru_cache(maxsize=None)
def case(dim, bitlevel):
    """one table, one batch of 130 wide-range vectors and the twin's result against EVERY row (plus a padding column at
    index ROWS) per (dim, bitlevel): each case below takes its vectors' rows and its candidates' columns of it, unchanged"""
    rng = np.random.default_rng(17 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    x = wide_values(rng, (max(NS), dim))
    full = np.concatenate([twin(packed, dim, bitlevel, x, None), np.zeros((max(NS), 1), np.float32)], axis=1)
    for a in (packed, x, full):
        a.setflags(write=False)
    return packed, x, full


def expected(full, n, cand):
    return np.ascontiguousarray(full[:n, :ROWS] if cand is None else full[:n][:, np.where(cand < 0, ROWS, cand)])


def device_project(emb, x, cand, dtype, slack=0):
    """the device form by hand: reserve, fill the staging views, launch, synchronise, read"""
    import torch
    n, m = len(x), emb.rows if cand is None else len(cand)
    x_t, cand_t, out = emb.staging_project(n + slack, m + slack, dtype)
    assert x_t.dtype == torch.float32 and x_t.shape == (n + slack, emb.dim) and cand_t.dtype == torch.int64 and out.is_cuda
    x_t[:n].copy_(torch.tensor(np.asarray(x, np.float32)))                  # (a copy: the cached vectors are read-only)
    if cand is not None:
        cand_t[:m].copy_(torch.from_numpy(np.asarray(cand, np.int64)))
    torch.cuda.synchronize()
    emb.project_device(n, m, cand is not None, dtype)
    emb.synchronize()
    return out[:n * m].view(n, m).clone()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", DIMS)
def test_every_form_equals_the_twin_in_float32(gpu, dim, bitlevel):
    """every n x every candidate list of the parametrisation, in the three forms"""
    import torch
    packed, x, full = case(dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    rng = np.random.default_rng(dim + bitlevel)
    for m in CANDS:
        cand = cand_list(rng, m)
        t_cand = None if cand is None else torch.from_numpy(cand)
        for n in NS:
            want = expected(full, n, cand)
            got = emb.project(x[:n], cand)
            assert got.dtype == np.float32 and same(got, want, "float32"), (n, m, "host form")
            assert same(device_project(emb, x[:n], cand, "float32"), want, "float32"), (n, m, "device form")
            got = emb.torch_project(torch.tensor(x[:n]), t_cand)
            assert got.is_cuda and got.dtype == torch.float32 and same(got, want, "float32"), (n, m, "torch")
    # the expected columns are the twin's own for a list too (the cache holds every row once): one direct comparison
    cand = cand_list(rng, 301)
    assert same(twin(packed, dim, bitlevel, x[:33], cand), expected(full, 33, cand), "float32")
    got = emb.torch_project(torch.tensor(x[:6].reshape(2, 3, dim)).cuda().double(), torch.from_numpy(cand).cuda().int())
    assert got.shape == (2, 3, 301) and same(got.reshape(6, 301), expected(full, 6, cand), "float32")     # any shape, cast
    emb.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("dim", [65, 200])
def test_sixteen_bit_outputs_are_the_twin_rounded_to_nearest_even(gpu, dim, dtype, bitlevel):
    """x = k / 64, |k| <= 4096: every partial sum is a multiple of 2^-6 below 2^24, so a non-zero |S q| is at least
    2^-6 / 4 and at most 64 * 200 * 3 * 0.75 < 65504: a normal float16 number.  Odd m: output rows start unaligned."""
    import torch
    rng = np.random.default_rng(90 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    x = (rng.integers(-4096, 4097, (67, dim)) / 64.0).astype(np.float32)
    for m in (33, 301, None, 64):
        cand = cand_list(rng, m)
        want = twin(packed, dim, bitlevel, x, cand)
        nz = np.abs(want[want != 0])
        assert nz.min() >= 2.0 ** -8 and nz.max() < 65504
        got = emb.project(x, cand, dtype)
        assert got.dtype == (np.float16 if dtype == "float16" else np.uint16) and same(got, want, dtype), (m, "host form")
        assert same(device_project(emb, x, cand, dtype), want, dtype), (m, "device form")
        got = emb.torch_project(torch.from_numpy(x), None if cand is None else torch.from_numpy(cand), tdtype(dtype))
        assert got.dtype == tdtype(dtype) and same(got, want, dtype), (m, "torch")
        for n in (1, 2, 3):                                                 # rows that start at odd and even elements
            assert same(emb.project(x[:n], cand, dtype), want[:n], dtype), (m, n)
    emb.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [65, 200])
def test_unit_vectors_read_the_table(gpu, dim, bitlevel):
    rng = np.random.default_rng(5 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    eye = np.eye(dim, dtype=np.float32)
    for dtype in DTYPES:
        rows = emb.lookup(np.arange(ROWS, dtype=np.int32), dtype)
        got = emb.project(eye, None, dtype)
        assert got.dtype == rows.dtype and np.array_equal(got.view(np.uint16), np.ascontiguousarray(rows.T).view(np.uint16)), dtype
    rc, want = host_lookup(packed, dim, bitlevel, np.arange(ROWS, dtype=np.int32))
    assert rc == 0 and same(emb.project(eye), np.ascontiguousarray(want.T), "float32")
    emb.close()


def test_a_large_call_is_chunked_and_keeps_its_bits(gpu):
    """n = 70 vectors against all of 300 000 rows at dim 64: 84 MB of float32, more than one 64 MiB chunk of the host
    form, cut between two candidate ranges.  4096 random positions, and the first and last row and column in full."""
    rng = np.random.default_rng(15)
    rows, dim, bitlevel, n = 300_000, 64, 2, 70
    packed = rng.integers(0, 2 ** 64, (rows, 2), dtype=np.uint64)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    x = wide_values(rng, (n, dim))
    emb.timing()
    got = emb.project(x)
    assert got.shape == (n, rows) and got.nbytes > (64 << 20) and emb.timing()[1] >= 2
    for i in (0, n - 1):
        assert same(got[i:i + 1], twin(packed, dim, bitlevel, x[i:i + 1], None), "float32"), i
    for j in (0, rows - 1):
        assert same(got[:, j:j + 1], twin(packed, dim, bitlevel, x, np.array([j], np.int32)), "float32"), j
    ii, jj = rng.integers(0, n, 4096), rng.integers(0, rows, 4096).astype(np.int32)
    want = twin(packed, dim, bitlevel, x, jj)                               # [n, 4096]: column k is candidate jj[k]
    assert np.array_equal(got[ii, jj].view(np.uint32), want[ii, np.arange(4096)].view(np.uint32))
    cand = np.concatenate([jj[:1000], [-1, rows - 1, 0]]).astype(np.int32)  # a list on the same handle
    assert same(emb.project(x[:3], cand), twin(packed, dim, bitlevel, x[:3], cand), "float32")
    emb.close()


def test_device_form_ignores_and_counts_what_is_out_of_range(gpu):
    """candidates >= rows and < 0 written into the staging (reserved a little larger, so that even an unclamped access
    would stay inside the allocations: a missing clamp shows as a wrong column or count)"""
    import torch
    rng = np.random.default_rng(19)
    dim, bitlevel = 200, 2
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    x = wide_values(rng, (70, dim))
    cand = rng.integers(0, ROWS, 500).astype(np.int64)
    cand[[3, 77]] = -1, -9
    bad = [17, 64, 400, 499]
    planted = cand.copy()
    planted[bad] = ROWS, ROWS + 5, 1 << 40, 2 ** 31
    clean = cand.copy()
    clean[bad] = -1
    want = twin(packed, dim, bitlevel, x, clean.astype(np.int32))
    for dtype in ("float32", "bfloat16"):
        got = device_project(emb, x, planted, dtype, slack=64)
        if dtype == "float32":
            assert same(got, want, "float32") and not got[:, bad + [3, 77]].any()
        assert emb.bad_ids() == len(bad) and emb.bad_ids() == 0
    with pytest.raises(w2b.W2bError) as e:
        emb.torch_project(torch.from_numpy(x), torch.from_numpy(planted))
    assert e.value.code == _lib.W2B_EINVAL and emb.bad_ids() == 0
    with pytest.raises(w2b.W2bError) as e:                                  # the host form refuses it before any launch
        emb.project(x, np.array([1, ROWS], np.int32))
    assert e.value.code == _lib.W2B_EINVAL
    with pytest.raises(w2b.W2bError) as e:
        emb.project(np.full((1, dim), np.inf, np.float32))
    assert e.value.code == _lib.W2B_EINVAL
    emb.close()


def test_reserve_project_has_buffers_of_its_own_and_refuses_more_than_it_holds(gpu):
    import torch
    rng = np.random.default_rng(23)
    dim, bitlevel = 65, 1
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    ids = rng.integers(0, ROWS, 50).astype(np.int32)
    ids_t, _, rows_out = emb.staging(50, 2)
    w_ptr = emb.reserve_weights(50)
    base = emb.reserve(50, 2)
    ids_t.copy_(torch.from_numpy(ids.astype(np.int64)))
    small = emb.reserve_project(4, 10)
    assert emb.reserve_project(2, 5) == small                               # asking for less changes nothing
    big = emb.reserve_project(40, ROWS + 10, "float32")                     # growing the projection's buffers ...
    assert emb.reserve_project(4, 10) == big and emb.reserve_project(40, ROWS) == big
    assert emb.reserve(50, 2) == base and emb.reserve_weights(50) == w_ptr  # ... leaves the others where they are
    torch.cuda.synchronize()
    emb.lookup_device(50)
    emb.synchronize()
    assert same(rows_out[:50].clone(), host_lookup(packed, dim, bitlevel, ids)[1], "float32")
    emb.reserve(5000, 100)                                                  # and the other way round
    assert emb.reserve_project(40, ROWS + 10) == big
    x = wide_values(rng, (40, dim))
    assert same(device_project(emb, x, None, "float32"), twin(packed, dim, bitlevel, x, None), "float32")
    for args in ((41, ROWS, True, "float32"), (40, ROWS + 11, True, "float32"), (40, ROWS + 10, True, "float32"),
                 (40, ROWS + 10, False, "float32"), (-1, 5, True, "float32"), (5, -1, True, "float32")):
        if args == (40, ROWS + 10, True, "float32"):
            emb.project_device(*args)                                       # exactly what was reserved is fine
            continue
        with pytest.raises(w2b.W2bError) as e:
            emb.project_device(*args)
        assert e.value.code == _lib.W2B_EINVAL, args
    emb.reserve_project(4, 4, "bfloat16")                                   # 16 bits of what was reserved: fits
    emb.project_device(40, ROWS + 10, True, "bfloat16")
    emb.synchronize()
    assert emb.bad_ids() >= 0
    fresh = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    fresh.reserve_project(4, 8, "bfloat16")
    with pytest.raises(w2b.W2bError) as e:                                  # float32 needs twice the bytes
        fresh.project_device(4, 8, True, "float32")
    assert e.value.code == _lib.W2B_EINVAL
    with pytest.raises(w2b.W2bError):
        fresh.project_device(4, 8, False, "bfloat16")                       # all rows need max_m >= rows
    with pytest.raises(ValueError):
        fresh.project(np.zeros((2, dim + 1), np.float32))
    fresh.close()
    emb.close()


def test_timing_counts_the_launches_and_the_stated_bytes(gpu):
    import torch
    rng = np.random.default_rng(29)
    dim, bitlevel = 65, 2
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    x = wide_values(rng, (33, dim))
    cand = cand_list(rng, 127)
    wpr = packed.shape[1]
    emb.timing()
    device_project(emb, x, cand, "float32")
    ms, launches, nbytes = emb.timing()
    assert launches == 1 and ms > 0 and nbytes == 33 * dim * 4 + 127 * wpr * 8 + 127 * 8 + 33 * 127 * 4
    device_project(emb, x, None, "bfloat16")
    emb.project(x, cand, "float16")
    ms, launches, nbytes = emb.timing()
    assert launches == 2 and nbytes == (33 * dim * 4 + ROWS * wpr * 8 + 33 * ROWS * 2) + \
        (33 * dim * 4 + 127 * wpr * 8 + 127 * 8 + 33 * 127 * 2)
    emb.project_device(0, 5)                                                # n == 0 and m == 0: nothing launched
    emb.project_device(5, 0)
    assert emb.project(np.zeros((0, dim), np.float32)).shape == (0, ROWS)
    assert emb.project(x, np.zeros(0, np.int32)).shape == (33, 0)
    assert emb.torch_project(torch.zeros(0, dim)).shape == (0, ROWS)
    assert emb.torch_project(torch.from_numpy(x), torch.zeros(0, dtype=torch.int64)).shape == (33, 0)
    assert emb.timing() == (0.0, 0, 0.0)
    emb.close()


def test_torch_is_an_independent_witness_at_two_bits(gpu):
    """|x| <= 8 integers, dim 200: every partial sum is an integer below 2^24 and the order is irrelevant, so torch's
    float64 x @ W.T on the expanded table, times 0.25, is the float32 output exactly"""
    import torch
    rng = np.random.default_rng(37)
    dim = 200
    packed, table = make_table(rng, ROWS, dim, 2)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=2)
    x = rng.integers(-8, 9, (130, dim)).astype(np.float32)
    W = torch.from_numpy(table).double().cuda()
    codes = W * 4.0                                                        # +-1 / +-3, exact
    want = ((torch.from_numpy(x).double().cuda() @ codes.T) * 0.25).float()
    got = emb.torch_project(torch.from_numpy(x))
    assert torch.equal(got.view(torch.int32), (want + 0.0).view(torch.int32))
    cand = torch.from_numpy(rng.integers(0, ROWS, 77))
    got = emb.torch_project(torch.from_numpy(x), cand)
    assert torch.equal(got.view(torch.int32), (want[:, cand.cuda()] + 0.0).view(torch.int32))
    emb.close()
