"""One run on the GPU: PackedEmbedding.torch_xent forward + backward against the composition torch_project -> torch cross_entropy
-> torch_backproject on the same handle, at 60 238 rows x 200 dims, n = 8192, both bitlevels: device time and peak device memory.
Run from the repository root; writes profiles/embed_xent_bench.json (DESIGN.md 3.6 quotes it)."""
import json, os, sys
import numpy as np
import torch
import torch.nn.functional as F
sys.path.insert(0, os.getcwd())
import word2bits_amd as w2b

ROWS, DIM, N, REPEATS = 60238, 200, 8192, 5
out = {"shape": {"rows": ROWS, "dim": DIM, "vectors": N, "values": "standard normal / 8"}, "warmup": 1, "repeats": REPEATS,
       "device": torch.cuda.get_device_name(0), "cases": {}}
rng = np.random.default_rng(0)
for bitlevel in (1, 2):
    wpr = (DIM + 63) // 64 * bitlevel
    packed = rng.integers(0, 2 ** 64, (ROWS, wpr), dtype=np.uint64)
    emb = w2b.PackedEmbedding(packed=packed, dim=DIM, bitlevel=bitlevel)
    x = torch.from_numpy((rng.standard_normal((N, DIM)) / 8).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, ROWS, N)).cuda()
    nseg = -(-ROWS // 256)
    res = {}
    # the new call
    ms_l, peak = [], 0
    for it in range(REPEATS + 1):
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); emb.timing()
        xt = x.clone().requires_grad_()
        loss = emb.torch_xent(xt, y, reduction="mean")
        loss.backward()
        torch.cuda.synchronize()
        ms, launches, _ = emb.timing()
        if it:
            ms_l.append(ms)
        peak = max(peak, torch.cuda.max_memory_allocated())
    lib = 2 * N * DIM * 4 + N * DIM * 4 + N * (8 + 8 + 12) + N * nseg * 12 + (64 << 20) // (4 * ROWS) * ROWS * 4
    res["xent"] = {"device_ms_median": float(np.median(ms_l)), "device_ms_min": float(min(ms_l)), "device_ms_max": float(max(ms_l)),
                   "launches": int(launches), "loss": float(loss.detach()), "torch_peak_bytes": int(peak), "library_buffer_bytes": int(lib),
                   "grad_abs_max": float(xt.grad.abs().max())}
    g_new = xt.grad.clone()
    # the composition the library offered before
    lib_l, torch_l, peak = [], [], 0
    for it in range(REPEATS + 1):
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); emb.timing()
        logits = emb.torch_project(x).requires_grad_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss2 = F.cross_entropy(logits, y)
        loss2.backward()
        b.record(); torch.cuda.synchronize()
        dx = emb.torch_backproject(logits.grad)
        torch.cuda.synchronize()
        ms, launches2, _ = emb.timing()
        if it:
            lib_l.append(ms); torch_l.append(a.elapsed_time(b))
        peak = max(peak, torch.cuda.max_memory_allocated())
        del logits, loss2
    lib2 = 2 * N * DIM * 4 + N * ROWS * 4 + N * ROWS * 4 + N * DIM * 4
    tot = [p + q for p, q in zip(lib_l, torch_l)]
    res["composition"] = {"library_ms_median": float(np.median(lib_l)), "torch_ms_median": float(np.median(torch_l)),
                          "device_ms_median": float(np.median(tot)), "device_ms_min": float(min(tot)), "device_ms_max": float(max(tot)),
                          "torch_peak_bytes": int(peak), "library_buffer_bytes": int(lib2),
                          "grad_max_difference": float((dx - g_new).abs().max())}
    res["time_vs_composition"] = res["xent"]["device_ms_median"] / res["composition"]["device_ms_median"]
    res["memory_vs_composition"] = (res["xent"]["torch_peak_bytes"] + lib) / (res["composition"]["torch_peak_bytes"] + lib2)
    out["cases"]["bitlevel%d" % bitlevel] = res
    emb.close()
    print(json.dumps(res), flush=True)
json.dump(out, open(os.path.join("profiles", "embed_xent_bench.json"), "w"))
