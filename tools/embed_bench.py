#!/usr/bin/env python3
"""Device time of the packed embedding layer (include/word2bits_embed.h) beside torch on the unpacked float32 table, in
one process on one GPU: synthetic 1-bit and 2-bit tables of 400 000 rows at dim 800 and 200, 1 M Zipf-distributed ids --
lookup to float32, lookup to bfloat16, and the mean over 32-id bags.  Ours runs in the device form (ids already in the
library's staging), HIP-event time from PackedEmbedding.timing(); torch runs index_select (then .to(bfloat16)) and
F.embedding_bag on its own resident copy of the table, torch.cuda.Event time.  Every case is warmed up, then the cases
are timed in turn, `--repeats` rounds (so that a drift of the machine falls on all of them alike); medians.  `bytes` is
what timing() counts: packed words read + output written.  One JSON line on stdout (and in --out).

--weighted times the weighted leg instead, on the same shapes: the weighted sum over the 32-id bags (per_sample_weights, SIF-like
weights a / (a + p(w)) of the Zipf ranks) beside F.embedding_bag(..., mode="sum", per_sample_weights=...) on the float table and
beside the unweighted bag kernel on the same ids.

    python tools/embed_bench.py --out profiles/embed_bench.json
    python tools/embed_bench.py --weighted --out profiles/embed_bench_weighted.json"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOF_GBS = 8000.0       # the HBM figure of the project's roofline


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=400_000)
    ap.add_argument("--ids", type=int, default=1_000_000)
    ap.add_argument("--bag", type=int, default=32)
    ap.add_argument("--dims", type=int, nargs="*", default=[800, 200])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--weighted", action="store_true", help="the weighted-bag leg instead of lookup / mean")
    ap.add_argument("--out")
    a = ap.parse_args()
    torch.cuda.init()                                        # torch's runtime first, then the library's (tests/conftest.py)
    import torch.nn.functional as F
    import word2bits_amd as w2b
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    p = 1.0 / np.arange(1, a.rows + 1)
    ids_np = rng.choice(a.rows, a.ids, p=p / p.sum()).astype(np.int64)               # Zipf: row = frequency rank
    n_bags = a.ids // a.bag
    off_np = (np.arange(n_bags + 1, dtype=np.int64) * a.bag)
    n_bag_ids = int(off_np[-1])
    ids_t, off_t = torch.from_numpy(ids_np).to(dev), torch.from_numpy(off_np).to(dev)
    pw = p / p.sum()
    w_np = (1e-3 / (1e-3 + pw[ids_np])).astype(np.float32)                            # SIF: a / (a + p(w)), a = 1e-3
    w_t = torch.from_numpy(w_np).to(dev)
    res = {"shape": {"rows": a.rows, "ids": a.ids, "bag": a.bag, "ids_distribution": "zipf(1)"}, "warmup": a.warmup,
           "repeats": a.repeats, "roof_gbs": ROOF_GBS, "device": torch.cuda.get_device_name(0), "cases": {}}

    def torch_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    for bitlevel in (1, 2):
        for dim in a.dims:
            wpr = w2b.packed_words_per_row(dim, bitlevel)
            packed = rng.integers(0, 2 ** 64, (a.rows, wpr), dtype=np.uint64)
            if dim % 64:
                packed[:, -bitlevel:] &= np.uint64((1 << (dim % 64)) - 1)
            free0 = torch.cuda.mem_get_info()[0]
            emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
            s_ids, s_off, _ = emb.staging(a.ids, n_bags, "float32")
            s_ids.copy_(ids_t)
            s_off.copy_(off_t)
            if a.weighted:
                emb.staging_weights(a.ids).copy_(w_t)
            torch.cuda.synchronize()
            ours_mem = free0 - torch.cuda.mem_get_info()[0]
            free1 = torch.cuda.mem_get_info()[0]
            table = torch.from_numpy(w2b.unpack_quantized(packed, dim, bitlevel)).to(dev)
            torch_mem_table = free1 - torch.cuda.mem_get_info()[0]

            def ours(fn):
                def run():
                    fn()
                    ms, _, nbytes = emb.timing()
                    return ms, nbytes
                return run
            keep = {}                                        # torch's result of the round, freed when the next one arrives

            def theirs(fn):
                def run():
                    keep.clear()
                    return torch_ms(lambda: keep.setdefault("x", fn())), None
                return run
            pairs = (("lookup_f32", "torch_index_select_f32"), ("lookup_bf16", "torch_index_select_to_bf16"),
                     ("bag_mean_f32", "torch_embedding_bag_mean_f32"))
            cases = {
                "lookup_f32": ours(lambda: emb.lookup_device(a.ids, "float32")),
                "torch_index_select_f32": theirs(lambda: torch.index_select(table, 0, ids_t)),
                "lookup_bf16": ours(lambda: emb.lookup_device(a.ids, "bfloat16")),
                "torch_index_select_to_bf16": theirs(lambda: torch.index_select(table, 0, ids_t).to(torch.bfloat16)),
                "bag_mean_f32": ours(lambda: emb.bag_device(n_bag_ids, n_bags, "mean", "float32")),
                "torch_embedding_bag_mean_f32": theirs(lambda: F.embedding_bag(ids_t[:n_bag_ids], table, off_t, mode="mean",
                                                                               include_last_offset=True)),
            }
            if a.weighted:
                pairs = (("bag_weighted_sum_f32", "torch_embedding_bag_weighted_sum_f32"), ("bag_weighted_sum_f32", "bag_sum_f32"))
                cases = {
                    "bag_weighted_sum_f32": ours(lambda: emb.bag_weighted_device(n_bag_ids, n_bags, "sum", "float32")),
                    "torch_embedding_bag_weighted_sum_f32": theirs(lambda: F.embedding_bag(
                        ids_t[:n_bag_ids], table, off_t, mode="sum", per_sample_weights=w_t[:n_bag_ids], include_last_offset=True)),
                    "bag_sum_f32": ours(lambda: emb.bag_device(n_bag_ids, n_bags, "sum", "float32")),
                }
            out = emb.staging(a.ids, n_bags, "float32")[2]
            if a.weighted:
                # the same sums up to the order and the rounding of the float operations: |sum| < 32, some sixty roundings of
                # at most 2^-20 each on the two sides
                emb.bag_weighted_device(n_bag_ids, n_bags, "sum", "float32")
                emb.synchronize()
                want = F.embedding_bag(ids_t[:n_bag_ids], table, off_t, mode="sum", per_sample_weights=w_t[:n_bag_ids],
                                       include_last_offset=True)
                assert torch.allclose(out[:n_bags], want, rtol=0, atol=2.0 ** -13)
                del want
            else:
                # same answers, or the times compare nothing (2-bit sums are exact in float32; the mean is one division)
                emb.lookup_device(a.ids, "float32")
                emb.synchronize()
                step = 100_000
                for i in range(0, a.ids, step):
                    assert torch.equal(out[i:i + step].view(torch.int32), table[ids_t[i:i + step]].view(torch.int32))
            assert emb.bad_ids() == 0
            for fn in cases.values():
                for _ in range(a.warmup):
                    fn()
            emb.timing()
            runs = {name: [] for name in cases}
            nbytes = {}
            for _ in range(a.repeats):
                for name, fn in cases.items():
                    ms, nb = fn()
                    runs[name].append(ms)
                    if nb is not None:
                        nbytes[name] = nb
            keep.clear()
            entry = {"packed_bytes": int(packed.nbytes), "float_table_bytes": int(a.rows * dim * 4),
                     "device_bytes_ours_table_and_staging": int(ours_mem), "device_bytes_torch_table": int(torch_mem_table)}
            for name, r in runs.items():
                entry[name] = {"median_ms": statistics.median(r), "min_ms": min(r), "max_ms": max(r)}
                if name in nbytes:
                    gbs = nbytes[name] / (statistics.median(r) * 1e-3) / 1e9
                    entry[name].update(bytes=nbytes[name], gbs=gbs, fraction_of_roof=gbs / ROOF_GBS)
            for o, t in pairs:
                entry[o]["time_vs_torch" if t.startswith("torch") else "time_vs_" + t] = entry[o]["median_ms"] / entry[t]["median_ms"]
            res["cases"]["bitlevel%d_dim%d" % (bitlevel, dim)] = entry
            emb.close()
            del table, out, s_ids, s_off
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
