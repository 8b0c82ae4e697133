#!/usr/bin/env python3
"""Device time of the packed embedding's back-projection (include/word2bits_embed.h, "Back-projection") beside the forward
projection of the same shape on the same handle and torch's float32 matmul on the expanded table, in one process on one GPU
per shape: the shapes of tools/embed_project_bench.py (synthetic 1-bit and 2-bit tables of 400 000 rows at dim 800 and 200,
n = 1024, every row and 8192 random candidates, Gaussian g and x).  Ours runs in the device form (g and the candidates already
in the library's staging), HIP-event time from PackedEmbedding.timing(); the forward is project_device with float32 output:
the same number of multiply-adds.  torch runs g @ W and g @ W[cand] (the gather inside the timed region) on its own resident
float32 table; torch.cuda.Event time.  The all-rows call is timed on both paths of the driver (W2B_EMBED_BACK_PATH: S in
registers, or the segments through the scratch and the finishing kernel) and once as the driver chooses, at n = 1024 and at
n = 32.  Every case is warmed up, then the cases are timed in turn, `--repeats` rounds (so that a drift of the machine falls
on all of them alike); medians, with min and max kept.  Per case of ours: the fraction of the f32 matrix peak (the figure of
bench.py --form eval) and the ratios to the forward and to torch.

Without --case the script is a driver that never touches the GPU itself: it starts one child per (bitlevel, dim), each under
its own time limit, and starts nothing more after a child that failed or ran out of time.

    python tools/embed_backproject_bench.py --out profiles/embed_backproject_bench.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FMA = 78.6e12      # multiply-adds/s of the f32 matrix pipe: 256 CU x 4 SIMD x 64 flop/clk x 2.4 GHz / 2 (bench.py --form eval)
PATH = "W2B_EMBED_BACK_PATH"


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
    n, m, rows, small = a.vectors, a.candidates, a.rows, 32
    cand_t = torch.from_numpy(rng.integers(0, rows, m).astype(np.int64)).to(dev)
    emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
    table = torch.from_numpy(w2b.unpack_quantized(packed, dim, bitlevel)).to(dev)
    torch.manual_seed(100 * dim + bitlevel)
    g_all = torch.randn(n, rows, device=dev)
    g_cand = torch.randn(n, m, device=dev)
    x_t = torch.randn(n, dim, device=dev)

    # same answers, or the times compare nothing: small integers make every sum exact, so float64 is the truth bit for bit
    q = np.array([0x3EAAAAAB if bitlevel == 1 else 0x3E800000], np.uint32).view(np.float32)[0]
    gi = torch.from_numpy(rng.integers(-8, 9, (64, m)).astype(np.float32)).to(dev)
    codes = torch.round(table[cand_t].double() / float(q))
    want = ((gi.double() @ codes) * float(q)).float()
    for path in ("registers", "scratch"):
        os.environ[PATH] = path
        got = emb.torch_backproject(gi, cand_t)
        assert torch.equal(got.view(torch.int32), (want + 0.0).view(torch.int32)), path
    del os.environ[PATH], gi, codes, want, got

    s_g, s_cand, _ = emb.staging_backproject(n, rows)
    p_x, p_cand, _ = emb.staging_project(n, rows, "float32")
    s_cand[:m].copy_(cand_t)
    p_cand[:m].copy_(cand_t)
    p_x.copy_(x_t)
    torch.cuda.synchronize()

    def torch_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    def back(g, cols, use_cand, path=None):
        """fill the staging with this case's g (dense [vectors][cols]: outside the timed region), then one launch"""
        def run():
            s_g[:g.numel()].copy_(g.reshape(-1))
            torch.cuda.synchronize()                         # the library's stream does not wait for torch's
            if path is None:
                os.environ.pop(PATH, None)
            else:
                os.environ[PATH] = path
            emb.backproject_device(g.shape[0], cols, use_cand)
            os.environ.pop(PATH, None)
            return emb.timing()[0]
        return run

    def forward(cols, use_cand):
        def run():
            emb.project_device(n, cols, use_cand, "float32")
            return emb.timing()[0]
        return run
    keep = {}                                                # torch's result of the round, freed when the next one arrives

    def theirs(fn):
        def run():
            keep.clear()
            return torch_ms(lambda: keep.setdefault("x", fn()))
        return run
    cases = {
        "back_all": back(g_all, rows, False),
        "back_all_registers": back(g_all, rows, False, "registers"),
        "back_all_scratch": back(g_all, rows, False, "scratch"),
        "forward_all": forward(rows, False),
        "torch_all": theirs(lambda: g_all @ table),
        "back_cand": back(g_cand, m, True),
        "forward_cand": forward(m, True),
        "torch_cand": theirs(lambda: g_cand @ table[cand_t]),
        "back_all_n32": back(g_all[:small], rows, False),
        "back_all_n32_registers": back(g_all[:small], rows, False, "registers"),
        "back_all_n32_scratch": back(g_all[:small], rows, False, "scratch"),
    }
    work = {"all": float(n) * rows * dim, "cand": float(n) * m * dim, "n32": float(small) * rows * dim}
    for fn in cases.values():
        for _ in range(a.warmup):
            fn()
    emb.timing()
    runs = {name: [] for name in cases}
    for _ in range(a.repeats):
        for name, fn in cases.items():
            runs[name].append(fn())
    keep.clear()
    assert emb.bad_ids() == 0
    entry = {"packed_bytes": int(packed.nbytes), "float_table_bytes": int(rows * dim * 4)}
    for name, r in runs.items():
        med = statistics.median(r)
        entry[name] = {"median_ms": med, "min_ms": min(r), "max_ms": max(r)}
        if not name.startswith("torch"):
            fma = work["n32" if "n32" in name else name.split("_")[1]]
            entry[name].update(fma_per_s=fma / (med * 1e-3), fraction_of_f32_matrix_peak=fma / (med * 1e-3) / PEAK_FMA)
    for name in runs:
        if name.startswith("back") and "n32" not in name:
            kind = name.split("_")[1]
            entry[name]["time_vs_forward"] = entry[name]["median_ms"] / entry["forward_" + kind]["median_ms"]
            entry[name]["time_vs_torch_f32"] = entry[name]["median_ms"] / entry["torch_" + kind]["median_ms"]
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
                sys.exit("embed_backproject_bench: bitlevel %d dim %d ran out of time; nothing more is started" % (bitlevel, dim))
            if p.returncode != 0:
                sys.exit("embed_backproject_bench: bitlevel %d dim %d failed (%d); nothing more is started" % (bitlevel, dim, p.returncode))
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
