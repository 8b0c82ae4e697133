#!/usr/bin/env python3
"""Device time of the packed embedding's projection (include/word2bits_embed.h, "Projection") beside torch's matmul on the
expanded float table, in one process on one GPU per shape: synthetic 1-bit and 2-bit tables of 400 000 rows at dim 800 and
200, n = 1024 Gaussian vectors, against every row and against 8192 random candidates, float32 and bfloat16 output.  Ours runs
in the device form (vectors and candidates already in the library's staging), HIP-event time from PackedEmbedding.timing()
(the operand kernel and the product: one launch).  torch runs x @ W.T and x @ W[cand].T (the gather inside the timed region)
on its own resident float32 table, and the same in bfloat16 on a bfloat16 copy of it; torch.cuda.Event time.  Every case is
warmed up, then the cases are timed in turn, `--repeats` rounds (so that a drift of the machine falls on all of them alike);
medians, with min and max kept.  Per case of ours: the fraction of the f32 matrix peak (the figure of bench.py --form eval),
the output write bandwidth, and the ratio to torch.

Without --case the script is a driver that never touches the GPU itself: it starts one child per (bitlevel, dim), each under
its own time limit, and starts nothing more after a child that failed or ran out of time.

    python tools/embed_project_bench.py --out profiles/embed_project_bench.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FMA = 78.6e12      # multiply-adds/s of the f32 matrix pipe: 256 CU x 4 SIMD x 64 flop/clk x 2.4 GHz / 2 (bench.py --form eval)


def run_case(a, bitlevel, dim):
    import torch
    torch.cuda.init()                                        # torch's runtime first, then the library's (tests/conftest.py)
    import word2bits_amd as w2b
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(100 * dim + bitlevel)
    wpr = w2b.packed_words_per_row(dim, bitlevel)
    packed = rng.integers(0, 2 ** 64, (a.rows, wpr), dtype=np.uint64)
    if dim % 64:
        packed[:, -bitlevel:] &= np.uint64((1 << (dim % 64)) - 1)
    n, m = a.vectors, a.candidates
    x_np = rng.standard_normal((n, dim)).astype(np.float32)
    cand_np = rng.integers(0, a.rows, m).astype(np.int64)
    free0 = torch.cuda.mem_get_info()[0]
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    s_x, s_cand, s_out = emb.staging_project(n, a.rows, "float32")
    ours_mem = free0 - torch.cuda.mem_get_info()[0]
    table = torch.from_numpy(w2b.unpack_quantized(packed, dim, bitlevel)).to(dev)
    table16 = table.to(torch.bfloat16)
    x_t, cand_t = torch.from_numpy(x_np).to(dev), torch.from_numpy(cand_np).to(dev)
    x16 = x_t.to(torch.bfloat16)

    # same answers, or the times compare nothing: small integers make every sum exact, so float64 is the truth bit for bit
    q = np.array([0x3EAAAAAB if bitlevel == 1 else 0x3E800000], np.uint32).view(np.float32)[0]
    xi = torch.from_numpy(rng.integers(-8, 9, (n, dim)).astype(np.float32)).to(dev)
    codes = torch.round(table[cand_t].double() / float(q))
    want = ((xi.double() @ codes.T) * float(q)).float()
    got = emb.torch_project(xi, cand_t)
    assert torch.equal(got.view(torch.int32), (want + 0.0).view(torch.int32))
    del xi, codes, want, got
    s_x, s_cand, s_out = emb.staging_project(n, a.rows, "float32")
    s_x.copy_(x_t)
    s_cand[:m].copy_(cand_t)
    torch.cuda.synchronize()

    def torch_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    def ours(fn):
        def run():
            fn()
            ms, _, nbytes = emb.timing()
            return ms, nbytes
        return run
    keep = {}                                                # torch's result of the round, freed when the next one arrives

    def theirs(fn):
        def run():
            keep.clear()
            return torch_ms(lambda: keep.setdefault("x", fn())), None
        return run
    cases = {
        "all_f32": ours(lambda: emb.project_device(n, a.rows, False, "float32")),
        "torch_all_f32": theirs(lambda: x_t @ table.T),
        "all_bf16": ours(lambda: emb.project_device(n, a.rows, False, "bfloat16")),
        "torch_all_bf16": theirs(lambda: x16 @ table16.T),
        "cand_f32": ours(lambda: emb.project_device(n, m, True, "float32")),
        "torch_cand_f32": theirs(lambda: x_t @ table[cand_t].T),
        "cand_bf16": ours(lambda: emb.project_device(n, m, True, "bfloat16")),
        "torch_cand_bf16": theirs(lambda: x16 @ table16[cand_t].T),
    }
    shapes = {"all": a.rows, "cand": m}
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
    assert emb.bad_ids() == 0
    entry = {"packed_bytes": int(packed.nbytes), "float_table_bytes": int(a.rows * dim * 4),
             "device_bytes_ours_table_and_staging": int(ours_mem)}
    for name, r in runs.items():
        med = statistics.median(r)
        entry[name] = {"median_ms": med, "min_ms": min(r), "max_ms": max(r)}
        if name in nbytes:
            cols = shapes[name.split("_")[0]]
            es = 4 if name.endswith("f32") else 2
            fma = float(n) * cols * dim
            entry[name].update(bytes=nbytes[name], fma_per_s=fma / (med * 1e-3), fraction_of_f32_matrix_peak=fma / (med * 1e-3) / PEAK_FMA,
                               output_write_gbs=float(n) * cols * es / (med * 1e-3) / 1e9)
    for name in nbytes:
        kind = name.split("_")[0]
        entry[name]["time_vs_torch_f32"] = entry[name]["median_ms"] / entry["torch_%s_f32" % kind]["median_ms"]
        entry[name]["time_vs_torch_bf16"] = entry[name]["median_ms"] / entry["torch_%s_bf16" % kind]["median_ms"]
    emb.close()
    print(json.dumps({"key": "bitlevel%d_dim%d" % (bitlevel, dim), "device": torch.cuda.get_device_name(0), "entry": entry}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=400_000)
    ap.add_argument("--vectors", type=int, default=1024)
    ap.add_argument("--candidates", type=int, default=8192)
    ap.add_argument("--dims", type=int, nargs="*", default=[800, 200])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for one (bitlevel, dim) child")
    ap.add_argument("--case", type=int, nargs=2, metavar=("BITLEVEL", "DIM"), help="run this one shape in this process")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        run_case(a, a.case[0], a.case[1])
        return
    res = {"shape": {"rows": a.rows, "vectors": a.vectors, "candidates": a.candidates, "values": "standard normal"},
           "warmup": a.warmup, "repeats": a.repeats, "f32_matrix_peak_fma_per_s": PEAK_FMA, "cases": {}}
    base = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--vectors", str(a.vectors), "--candidates",
            str(a.candidates), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
    for bitlevel in (1, 2):
        for dim in a.dims:
            try:
                p = subprocess.run(base + ["--case", str(bitlevel), str(dim)], stdout=subprocess.PIPE, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                sys.exit("embed_project_bench: bitlevel %d dim %d ran out of time; nothing more is started" % (bitlevel, dim))
            if p.returncode != 0:
                sys.exit("embed_project_bench: bitlevel %d dim %d failed (%d); nothing more is started" % (bitlevel, dim, p.returncode))
            got = json.loads(p.stdout.decode().strip().splitlines()[-1])
            res["device"] = got["device"]
            res["cases"][got["key"]] = got["entry"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
