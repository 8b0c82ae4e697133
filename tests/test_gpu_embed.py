"""Packed embedding layer on the GPU (include/word2bits_embed.h): the host form, the device form and the torch front
against the host twins of tests/test_embed_host.py (which ties them to the numpy definition), bit for bit; bf16 / f16
against the twins' float32 result rounded to nearest even.  No tolerance anywhere."""
import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from test_embed_host import host_bag, host_lookup, make_table

pytestmark = pytest.mark.gpu
DIMS = [1, 3, 64, 65, 200, 800]
DTYPES = ["float32", "bfloat16", "float16"]
ROWS = 300


def rounded(want32, dtype):
    """the float32 truth as the bit patterns of `dtype`"""
    if dtype == "float32":
        return want32.view(np.uint32)
    if dtype == "float16":
        return want32.astype(np.float16).view(np.uint16)
    u = want32.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bits_of(x, dtype):
    """bit patterns of a numpy result of PackedEmbedding or of a torch tensor"""
    if not isinstance(x, np.ndarray):
        import torch
        x = x.view(torch.int16).cpu().numpy() if x.dtype == torch.bfloat16 else x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint32 if dtype == "float32" else np.uint16)


def tdtype(dtype):
    import torch
    return getattr(torch, dtype)


def same(got, want32, dtype):
    g, w = bits_of(got, dtype), rounded(want32, dtype)
    return g.shape == w.shape and np.array_equal(g, w)


def device_lookup(emb, ids, dtype):
    """the device form by hand: reserve, fill the staging through its torch view, launch, synchronise, read"""
    import torch
    ids_t, _, out = emb.staging(len(ids), 0, dtype)
    ids_t.copy_(torch.from_numpy(ids.astype(np.int64)))
    torch.cuda.synchronize()
    emb.lookup_device(len(ids), dtype)
    emb.synchronize()
    return out[:len(ids)].clone()


def device_bag(emb, ids, offsets, mode, dtype):
    import torch
    ids_t, off_t, out = emb.staging(len(ids), len(offsets) - 1, dtype)
    ids_t.copy_(torch.from_numpy(ids.astype(np.int64)))
    off_t.copy_(torch.from_numpy(offsets))
    torch.cuda.synchronize()
    emb.bag_device(len(ids), len(offsets) - 1, mode, dtype)
    emb.synchronize()
    return out[:len(offsets) - 1].clone()


def skewed_bags(rng, rows, total=70_000):
    """a thousand bags of 0 to 3 ids with one bag of 65 000 ids between them, a bag that is all padding, and a last bag
    that ends at n_ids"""
    lens = rng.integers(0, 4, 1000).tolist()
    lens.insert(500, 65_000)
    lens.insert(700, 6)                                                    # the padding bag
    lens.append(total - sum(lens))
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = rng.integers(-1, rows, total).astype(np.int32)
    ids[offsets[700]:offsets[701]] = -1
    assert offsets[-1] == total and lens[-1] > 1024
    return ids, offsets


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", DIMS)
def test_lookup_equals_the_host_twin_in_every_form(gpu, dim, bitlevel):
    import torch
    rng = np.random.default_rng(7 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    assert (emb.rows, emb.dim, emb.bitlevel) == (ROWS, dim, bitlevel) and emb.word(0) is None and emb.search(b"x") == -1
    for n in (1, 63, 64, 257, 5000):
        ids = rng.integers(-1, ROWS, n).astype(np.int32)
        ids[-1] = ROWS - 1
        rc, want = host_lookup(packed, dim, bitlevel, ids)
        assert rc == 0
        for dtype in DTYPES:
            assert same(emb.lookup(ids, dtype), want, dtype), (n, dtype, "host form")
            assert same(device_lookup(emb, ids, dtype), want, dtype), (n, dtype, "device form")
            got = emb.torch_lookup(torch.from_numpy(ids), tdtype(dtype))
            assert got.dtype == tdtype(dtype) and got.is_cuda and same(got, want, dtype), (n, dtype, "torch")
    got = emb.torch_lookup(torch.from_numpy(ids[:12].reshape(3, 4)).cuda())          # ids on the device, any shape
    assert got.shape == (3, 4, dim) and same(got.reshape(12, dim), want[:12], "float32")
    emb.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", DIMS)
def test_bags_equal_the_host_twin_in_every_form(gpu, dim, bitlevel):
    import torch
    rng = np.random.default_rng(11 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    ids, offsets = skewed_bags(rng, ROWS)
    for code, mode in enumerate(("sum", "mean")):
        rc, want = host_bag(packed, dim, bitlevel, ids, offsets, code)
        assert rc == 0 and np.all(want[700].view(np.uint32) == 0)
        for dtype in DTYPES:
            assert same(emb.bag(ids, offsets, mode, dtype), want, dtype), (mode, dtype, "host form")
            assert same(device_bag(emb, ids, offsets, mode, dtype), want, dtype), (mode, dtype, "device form")
            got = emb.torch_bag(torch.from_numpy(ids), torch.from_numpy(offsets), mode, tdtype(dtype))
            assert got.dtype == tdtype(dtype) and same(got, want, dtype), (mode, dtype, "torch")
    emb.close()


def test_torch_is_an_independent_witness_at_two_bits(gpu):
    """bitlevel 2, float32: multiples of .25 add exactly, so torch's own embedding / embedding_bag on the unpacked table
    must give the same bits"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    dim = 200
    packed, table = make_table(rng, ROWS, dim, 2)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=2)
    ids, offsets = skewed_bags(rng, ROWS)
    ids = np.abs(ids)                                                      # torch has no padding id < 0
    t_ids, t_off, t_table = torch.from_numpy(ids.astype(np.int64)), torch.from_numpy(offsets), torch.from_numpy(table)
    got = emb.torch_lookup(t_ids)
    assert torch.equal(got.cpu().view(torch.int32), F.embedding(t_ids, t_table).view(torch.int32))
    got = emb.torch_bag(t_ids, t_off, "sum")
    want = F.embedding_bag(t_ids, t_table, t_off, mode="sum", include_last_offset=True)
    assert torch.equal(got.cpu().view(torch.int32), (want + 0.0).view(torch.int32))
    emb.close()


def test_device_form_ignores_and_counts_what_is_out_of_range(gpu):
    """ids `rows` and `rows + 5` and one bag bound of n_ids + 3 written into the staging buffers (reserved a little larger,
    so that even an unclamped access would stay inside the allocations: a missing clamp shows as a wrong row or count)"""
    import torch
    rng = np.random.default_rng(8)
    dim = 200
    packed, _ = make_table(rng, ROWS, dim, 1)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=1)
    n = 500
    ids = rng.integers(0, ROWS, n).astype(np.int32)
    clean = ids.copy()
    clean[[17, 400]] = -1                                                  # what the planted ids must behave like
    planted = ids.astype(np.int64)
    planted[17], planted[400] = ROWS, ROWS + 5
    rc, want = host_lookup(packed, dim, 1, clean)
    ids_t, _, out = emb.staging(n + 64, 0, "float32")
    ids_t[:n].copy_(torch.from_numpy(planted))
    torch.cuda.synchronize()
    emb.lookup_device(n, "float32")
    emb.synchronize()
    assert same(out[:n].clone(), want, "float32") and not out[17].any() and not out[400].any()
    assert emb.bad_ids() == 2 and emb.bad_ids() == 0
    with pytest.raises(w2b.W2bError) as e:
        emb.torch_lookup(torch.from_numpy(planted))
    assert e.value.code == _lib.W2B_EINVAL and emb.bad_ids() == 0
    offsets = np.array([0, 10, 10, 300, n], np.int64)
    rc, want = host_bag(packed, dim, 1, clean, offsets, 1)
    bad_off = offsets.copy()
    bad_off[-1] = n + 3                                                    # clamped back to n_ids
    ids_t, off_t, out = emb.staging(n + 64, 4, "float32")
    ids_t[:n].copy_(torch.from_numpy(planted))
    ids_t[n:].fill_(1)
    off_t.copy_(torch.from_numpy(bad_off))
    torch.cuda.synchronize()
    emb.bag_device(n, 4, "mean", "float32")
    emb.synchronize()
    assert same(out[:4].clone(), want, "float32")
    assert emb.bad_ids() == 3 and emb.bad_ids() == 0
    with pytest.raises(w2b.W2bError) as e:                                 # more than was reserved: refused on the host
        emb.lookup_device(n + 65, "float32")
    assert e.value.code == _lib.W2B_EINVAL
    emb.close()


def test_output_beyond_4_gib(gpu):
    """dim = 800, 1 400 000 ids: 4.48 GB of float32 through the device form, compared on the device in slices"""
    import torch
    rng = np.random.default_rng(12)
    dim, n = 800, 1_400_000
    packed, table = make_table(rng, ROWS, dim, 1)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=1)
    ids = torch.from_numpy(rng.integers(0, ROWS, n).astype(np.int64)).cuda()
    ids[-1], ids[-2] = ROWS - 1, 0
    out = emb.torch_lookup(ids, copy=False)
    assert out.shape == (n, dim) and out.numel() * 4 > (1 << 32)
    table_dev = torch.from_numpy(table).cuda()
    step = 100_000
    for a in range(0, n, step):
        assert torch.equal(out[a:a + step].view(torch.int32), table_dev[ids[a:a + step]].view(torch.int32)), a
    assert torch.equal(out[-1].cpu(), torch.from_numpy(table[ROWS - 1]))
    del out
    emb.close()


def test_one_million_rows_stay_packed(gpu, tmp_path):
    """V = 1 000 000, dim = 200, bitlevel 1 from a .w2bp written here: 32 MB of packed rows where the float table would be
    800 MB.  Allowance as for the packed evaluator: 64 MiB for the allocator's granularity, the stream and the staging."""
    import torch
    V, D = 1_000_000, 200
    rng = np.random.default_rng(77)
    wpr = (D + 63) // 64
    packed = rng.integers(0, 2 ** 64, (V, wpr), dtype=np.uint64)
    packed[:, -1] &= np.uint64((1 << (D - 64 * (wpr - 1))) - 1)       # padding bits are zero in the file
    with open(str(tmp_path / "big.w2bp"), "wb") as f:
        f.write(b"W2BP1 %d %d 1\n" % (V, D))
        f.write(b"".join(b"w%d\n" % i for i in range(V)))
        f.write(packed.astype("<u8").tobytes())
    free0 = torch.cuda.mem_get_info()[0]
    emb = w2b.PackedEmbedding(str(tmp_path / "big.w2bp"))
    ids = rng.integers(0, V, 1000).astype(np.int32)
    ids[:3] = [0, V - 1, -1]
    got = emb.lookup(ids)
    used = free0 - torch.cuda.mem_get_info()[0]
    print("device footprint %.1f MiB for %.1f MiB of packed rows" % (used / 2 ** 20, packed.nbytes / 2 ** 20))
    assert used < 2 * packed.nbytes + (64 << 20)
    rc, want = host_lookup(packed, D, 1, ids)
    assert rc == 0 and same(got, want, "float32")
    assert (emb.rows, emb.dim, emb.bitlevel) == (V, D, 1)
    assert emb.word(V - 1) == b"w%d" % (V - 1) and emb.search(b"w123456") == 123456 and emb.search("nope") == -1
    emb.close()
    emb = w2b.PackedEmbedding(str(tmp_path / "big.w2bp"), threshold=1000)
    assert emb.rows == 1000 and emb.search(b"w1000") == -1
    with pytest.raises(w2b.W2bError):
        emb.lookup(np.array([1000], np.int32))
    assert same(emb.lookup(np.array([999], np.int32)), host_lookup(packed, D, 1, np.array([999], np.int32))[1], "float32")
    emb.close()


def test_growing_the_staging_timing_and_empty_calls(gpu):
    import torch
    rng = np.random.default_rng(21)
    dim = 65
    packed, _ = make_table(rng, ROWS, dim, 2)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=2)
    ids = rng.integers(-1, ROWS, 3000).astype(np.int32)
    offsets = np.array([0, 1, 1, 1500, 3000], np.int64)
    want_l, want_b = host_lookup(packed, dim, 2, ids)[1], host_bag(packed, dim, 2, ids, offsets, 1)[1]
    small = emb.reserve(10, 1)
    assert emb.reserve(5, 0) == small                                      # asking for less changes nothing
    assert same(device_lookup(emb, ids[:10], "float32"), want_l[:10], "float32")
    emb.timing()
    first = (device_lookup(emb, ids, "float32"), device_bag(emb, ids, offsets, "mean", "float32"))    # both grow the buffers
    big = emb.reserve(100_000, 5000, "float32")
    again = (device_lookup(emb, ids, "float32"), device_bag(emb, ids, offsets, "mean", "float32"))
    assert emb.reserve(3000, 4) == big
    for got in (first, again):
        assert same(got[0], want_l, "float32") and same(got[1], want_b, "float32")
    ms, launches, nbytes = emb.timing()
    wpr = packed.shape[1]
    assert launches == 4 and ms > 0 and nbytes == 2 * (3000 * wpr * 8 + 3000 * dim * 4) + 2 * (3000 * wpr * 8 + 4 * dim * 4)
    assert emb.timing() == (0.0, 0, 0.0)
    assert emb.lookup(np.zeros(0, np.int32)).shape == (0, dim)             # n == 0 and n_bags == 0 are fine
    assert emb.bag(np.zeros(0, np.int32), np.zeros(1, np.int64)).shape == (0, dim)
    emb.lookup_device(0)
    emb.bag_device(0, 0)
    assert emb.torch_lookup(torch.zeros(0, dtype=torch.int64)).shape == (0, dim)
    assert emb.torch_bag(torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)).shape == (0, dim)
    empty = emb.torch_bag(torch.zeros(0, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), "mean")     # bags without ids
    assert empty.shape == (2, dim) and not empty.any() and emb.timing()[1] == 1
    with pytest.raises(w2b.W2bError) as e:
        emb.lookup(np.array([ROWS], np.int32))
    assert e.value.code == _lib.W2B_EINVAL
    emb.close()
