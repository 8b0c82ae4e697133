"""Weighted bag pooling on the GPU (include/word2bits_embed.h, "Weighted bag"): the host form, the device form and the
torch front against the host twin of tests/test_embed_weighted_host.py (which ties it to the numpy definition), bit for
bit; bf16 / f16 against the twin's float32 result rounded to nearest even.  No tolerance anywhere."""
import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from test_embed_host import make_table
from test_embed_weighted_host import LENGTHS, dyadic_weights, host_bag_weighted, make_bags
from test_gpu_embed import DTYPES, ROWS, same, skewed_bags, tdtype

pytestmark = pytest.mark.gpu
MODES = ("sum", "mean")


def wide_weights(rng, n):
    """the whole allowed range: random sign, exponent -60 .. 59, random mantissa, and some zeros of either sign"""
    bits = (rng.integers(0, 2, n).astype(np.uint32) << 31) | ((127 + rng.integers(-60, 60, n)).astype(np.uint32) << 23) | \
        rng.integers(0, 1 << 23, n).astype(np.uint32)
    bits[rng.random(n) < 0.03] &= np.uint32(0x80000000)
    w = bits.view(np.float32)
    assert np.isfinite(w).all() and (w == 0).any() and np.abs(w).max() < 2.0 ** 60 and np.abs(w[w != 0]).min() >= 2.0 ** -60
    return w


def twin(packed, dim, bitlevel, ids, weights, offsets, mode):
    rc, want = host_bag_weighted(packed, dim, bitlevel, ids, weights, offsets, MODES.index(mode))
    assert rc == 0
    return want


def device_bag_weighted(emb, ids, weights, offsets, mode, dtype, n_ids=None, slack=0):
    """the device form by hand: reserve, fill the three staging views, launch, synchronise, read"""
    import torch
    n = len(ids) if n_ids is None else n_ids
    nb = len(offsets) - 1
    ids_t, off_t, out = emb.staging(n + slack, nb, dtype)
    w_t = emb.staging_weights(n + slack)
    assert w_t.dtype == torch.float32 and w_t.shape == (n + slack,) and w_t.is_cuda
    ids_t.fill_(1)
    w_t.fill_(1.0)
    ids_t[:len(ids)].copy_(torch.from_numpy(np.asarray(ids, np.int64)))
    w_t[:len(ids)].copy_(torch.from_numpy(np.asarray(weights, np.float32)))
    off_t.copy_(torch.from_numpy(np.asarray(offsets, np.int64)))
    torch.cuda.synchronize()
    emb.bag_weighted_device(n, nb, mode, dtype)
    emb.synchronize()
    return out[:nb].clone()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dim", [1, 3, 64, 65, 200, 1089])
def test_host_form_equals_the_twin_over_the_whole_weight_range(gpu, dim, bitlevel):
    rng = np.random.default_rng(13 * dim + bitlevel)
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    ids, offsets = make_bags(rng, ROWS, LENGTHS + [3100])
    weights = wide_weights(rng, len(ids))
    for mode in MODES:
        got = emb.bag(ids, offsets, mode, per_sample_weights=weights)
        assert same(got, twin(packed, dim, bitlevel, ids, weights, offsets, mode), "float32"), mode
    emb.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_sixteen_bit_outputs_are_the_twin_rounded_to_nearest_even(gpu, dtype, bitlevel):
    """weights k / 64, |k| <= 4096, bags of at most 64 ids: a non-zero |result| is at least 2^-6 / 4 / 64 = 2^-14 and
    at most 64 * 64 * 3, so it is a normal float16 number"""
    rng = np.random.default_rng(90 + bitlevel)
    dim = 200
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    ids, offsets = make_bags(rng, ROWS, [0, 1, 2, 3, 4, 5, 31, 63, 64] * 3)
    weights = dyadic_weights(rng, len(ids), kmax=4096)
    for mode in MODES:
        want = twin(packed, dim, bitlevel, ids, weights, offsets, mode)
        nz = np.abs(want[want != 0])
        assert nz.min() >= 2.0 ** -14 and nz.max() < 65504
        assert same(emb.bag(ids, offsets, mode, dtype, per_sample_weights=weights), want, dtype), mode
        assert same(device_bag_weighted(emb, ids, weights, offsets, mode, dtype), want, dtype), mode
    emb.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_device_form_and_torch_front(gpu, bitlevel):
    import torch
    rng = np.random.default_rng(70 + bitlevel)
    dim = 65
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    ids, offsets = make_bags(rng, ROWS)
    weights = wide_weights(rng, len(ids))
    t_ids, t_off, t_w = torch.from_numpy(ids), torch.from_numpy(offsets), torch.from_numpy(weights)
    for mode in MODES:
        want = twin(packed, dim, bitlevel, ids, weights, offsets, mode)
        assert same(device_bag_weighted(emb, ids, weights, offsets, mode, "float32"), want, "float32"), mode
        got = emb.torch_bag(t_ids, t_off, mode, per_sample_weights=t_w)
        assert got.is_cuda and got.dtype == torch.float32 and same(got, want, "float32"), (mode, "cpu tensors")
        got = emb.torch_bag(t_ids.cuda(), t_off.cuda(), mode, per_sample_weights=t_w.cuda())
        assert same(got, want, "float32"), (mode, "cuda tensors")
        got = emb.torch_bag(t_ids, t_off.cuda(), mode, per_sample_weights=t_w.double())           # cast to float32: exact
        assert same(got, want, "float32"), (mode, "float64 weights")
        got = emb.torch_bag(t_ids, t_off, mode, torch.bfloat16, per_sample_weights=t_w.double().cuda())
        assert got.dtype == torch.bfloat16 and same(got, want, "bfloat16"), (mode, "bfloat16 out")
    with pytest.raises(ValueError):
        emb.torch_bag(t_ids, t_off, per_sample_weights=t_w[:-1])
    with pytest.raises(w2b.W2bError) as e:                                  # no weights reserved for that many ids
        emb.staging(len(ids) + 10, len(offsets) - 1)
        emb.bag_weighted_device(len(ids) + 10, len(offsets) - 1)
    assert e.value.code == _lib.W2B_EINVAL
    w_ptr = emb.reserve_weights(len(ids))
    emb.reserve(4 * len(ids), len(offsets) + 5)                             # growing the others leaves the weights where they are
    assert emb.reserve_weights(10) == w_ptr
    emb.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_unit_weights_equal_the_unweighted_kernels(gpu, bitlevel):
    """every partial sum is an integer below 2^24: the float chains and the bit counters must agree bit for bit, on a
    thousand short bags with one of 65 000 ids between them"""
    rng = np.random.default_rng(50 + bitlevel)
    dim = 200
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    ids, offsets = skewed_bags(rng, ROWS)
    ones = np.ones(len(ids), np.float32)
    for mode in MODES:
        for dtype in DTYPES:
            want = emb.bag(ids, offsets, mode, dtype)
            got = emb.bag(ids, offsets, mode, dtype, per_sample_weights=ones)
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint16), want.view(np.uint16)), (mode, dtype)
    emb.close()


def test_the_order_of_a_bag_is_kept(gpu):
    rng = np.random.default_rng(61)
    dim, bitlevel = 200, 2
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    n = 2500
    ids = rng.integers(0, ROWS, n).astype(np.int32)
    weights = wide_weights(rng, n)
    offsets = np.array([0, 700, n], np.int64)                               # a one-chain bag and a segmented one
    perm = np.concatenate([rng.permutation(700), 700 + rng.permutation(n - 700)])
    first = emb.bag(ids, offsets, "sum", per_sample_weights=weights)
    second = emb.bag(ids[perm], offsets, "sum", per_sample_weights=weights[perm])
    assert same(first, twin(packed, dim, bitlevel, ids, weights, offsets, "sum"), "float32")
    assert same(second, twin(packed, dim, bitlevel, ids[perm], weights[perm], offsets, "sum"), "float32")
    for b in (0, 1):
        assert (first[b].view(np.uint32) != second[b].view(np.uint32)).any(), b
    emb.close()


def test_device_form_ignores_and_counts_what_is_out_of_range(gpu):
    """ids >= rows, refused weights on valid ids and a bag bound beyond n_ids written into the staging buffers (reserved
    a little larger, so that even an unclamped access would stay inside the allocations: a missing clamp shows as a wrong
    value or count)"""
    import torch
    rng = np.random.default_rng(9)
    dim, bitlevel = 200, 2
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    n = 3000
    ids = rng.integers(0, ROWS, n).astype(np.int32)
    ids[[5, 1500]] = -1
    weights = wide_weights(rng, n)
    offsets = np.array([0, 10, 10, 300, 1700, n], np.int64)                 # the bag 300 .. 1700 takes the segment path
    planted_ids, planted_w = ids.astype(np.int64), weights.copy()
    planted_ids[[17, 400, 2999]] = ROWS, ROWS + 5, 1 << 40
    bad_w = {3: np.nan, 350: np.inf, 1400: -np.inf, 1699: 2.0 ** 61, 2000: -(2.0 ** -61), 2500: 1e-45}
    for i, v in bad_w.items():
        assert ids[i] >= 0
        planted_w[i] = v
    planted_w[[5, 1500]] = np.nan, 2.0 ** 100                               # on padding ids: ignored, not counted
    clean = ids.copy()
    clean[[17, 400, 2999] + list(bad_w)] = -1
    bad_off = offsets.copy()
    bad_off[-1] = n + 3                                                     # clamped back to n_ids
    for mode in MODES:
        want = twin(packed, dim, bitlevel, clean, weights, offsets, mode)
        got = device_bag_weighted(emb, planted_ids, planted_w, bad_off, mode, "float32", n_ids=n, slack=64)
        assert same(got, want, "float32"), mode
        assert emb.bad_ids() == 3 + len(bad_w) + 1 and emb.bad_ids() == 0
    with pytest.raises(w2b.W2bError) as e:
        emb.torch_bag(torch.from_numpy(planted_ids), torch.from_numpy(offsets), per_sample_weights=torch.from_numpy(weights))
    assert e.value.code == _lib.W2B_EINVAL and emb.bad_ids() == 0
    with pytest.raises(w2b.W2bError) as e:
        emb.torch_bag(torch.from_numpy(ids), torch.from_numpy(offsets), per_sample_weights=torch.from_numpy(planted_w))
    assert e.value.code == _lib.W2B_EINVAL and emb.bad_ids() == 0
    emb.close()


def test_overlapping_long_bags_find_the_list_full_and_are_still_pooled_by_segments(gpu):
    """bounds that only a damaged offsets buffer can hold: three bags of three segments over the same 2200 ids, where the
    scratch has rows for five segments.  The bags that find it full are walked by their own workgroup, segment by segment:
    the same result."""
    rng = np.random.default_rng(10)
    dim, bitlevel = 200, 1
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    n = 2200
    ids = rng.integers(-1, ROWS, n).astype(np.int32)
    weights = wide_weights(rng, n)
    planted = np.array([0, n, 50, n, 10, n], np.int64)                      # bags 1 and 3 end before they start: empty, counted
    cuts = [(0, n), (n, n), (50, n), (n, n), (10, n)]
    c_ids = np.concatenate([ids[a:b] for a, b in cuts])
    c_w = np.concatenate([weights[a:b] for a, b in cuts])
    c_off = np.concatenate([[0], np.cumsum([b - a for a, b in cuts])]).astype(np.int64)
    for mode in MODES:
        want = twin(packed, dim, bitlevel, c_ids, c_w, c_off, mode)
        got = device_bag_weighted(emb, ids, weights, planted, mode, "float32", slack=64)
        assert same(got, want, "float32"), mode
        assert emb.bad_ids() == 2
    emb.close()


def test_a_large_call_is_chunked_by_whole_bags(gpu):
    """25 000 two-id bags at dim 800: 80 MB of float32 output, more than one 64 MiB chunk of the host form"""
    rng = np.random.default_rng(14)
    dim, bitlevel, nb = 800, 1, 25_000
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    ids = rng.integers(-1, ROWS, 2 * nb).astype(np.int32)
    weights = wide_weights(rng, 2 * nb)
    offsets = (2 * np.arange(nb + 1)).astype(np.int64)
    emb.timing()
    got = emb.bag(ids, offsets, "mean", per_sample_weights=weights)
    assert got.nbytes > (64 << 20) and emb.timing()[1] >= 2
    assert same(got, twin(packed, dim, bitlevel, ids, weights, offsets, "mean"), "float32")
    emb.close()


def test_timing_counts_the_launch_and_the_weights(gpu):
    rng = np.random.default_rng(22)
    dim, bitlevel = 65, 2
    packed, _ = make_table(rng, ROWS, dim, bitlevel)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    ids = rng.integers(-1, ROWS, 3000).astype(np.int32)
    weights = wide_weights(rng, 3000)
    offsets = np.array([0, 1, 1, 1500, 3000], np.int64)
    emb.timing()
    device_bag_weighted(emb, ids, weights, offsets, "mean", "float32")
    ms, launches, nbytes = emb.timing()
    wpr = packed.shape[1]
    assert launches == 1 and ms > 0 and nbytes == 3000 * wpr * 8 + 4 * 3000 + 4 * dim * 4
    emb.bag_weighted_device(0, 0)                                          # n_bags == 0: nothing launched
    assert emb.bag(np.zeros(0, np.int32), np.zeros(1, np.int64), per_sample_weights=np.zeros(0, np.float32)).shape == (0, dim)
    assert emb.timing() == (0.0, 0, 0.0)
    emb.close()
