"""One run on the GPU: PackedEmbedding.topk_device against the composition project_device -> torch.topk on the same handle (what
the library offered before), all rows, at 60 238 rows x 200 dims and 400 000 rows x 800 dims, both bitlevels, n of 32, 1024, 8192
and k of 1, 8, 64: device time (the library's events for its launches, torch's events for torch.topk; medians of 7 interleaved
rounds after 2 warm-up rounds, one process) and peak device memory (torch's max_memory_allocated plus the library's buffers by
their reserve sizes).  Run from the repository root; writes profiles/embed_topk_bench.json (DESIGN.md 3.6 quotes it)."""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.getcwd())
import word2bits_amd as w2b

SHAPES = [(60238, 200), (400000, 800)]
NS, KS, WARMUP, ROUNDS = (32, 1024, 8192), (1, 8, 64), 2, 7
SCRATCH = 64 << 20


def topk_bytes(rows, dim, n, k):
    """the library's device buffers of a topk_device call of n vectors against all rows (include/word2bits_embed.h)"""
    per_vector = -(-rows // 64) * 8 + 512 * k + 16
    sv = min(n, max(64, SCRATCH // per_vector // 64 * 64))
    return 2 * n * dim * 4 + 16 * rows + n * k * 12 + sv * per_vector


def composition_bytes(rows, dim, n):
    return 2 * n * dim * 4 + 8 * rows + n * rows * 4


out = {"shapes": SHAPES, "vectors": NS, "k": KS, "values": "standard normal", "candidates": "all rows", "warmup": WARMUP,
       "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "cases": []}
rng = np.random.default_rng(0)
for rows, dim in SHAPES:
    for bitlevel in (1, 2):
        wpr = (dim + 63) // 64 * bitlevel
        packed = rng.integers(0, 2 ** 64, (rows, wpr), dtype=np.uint64)
        emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
        x = torch.from_numpy(rng.standard_normal((max(NS), dim)).astype(np.float32)).cuda()
        x_t, _, vals, pos = emb.staging_topk(max(NS), rows, max(KS))
        x_p, _, logits = emb.staging_project(max(NS), rows)
        x_t.copy_(x)
        x_p.copy_(x)
        torch.cuda.synchronize()
        times = {(n, k): {"topk": [], "project": [], "torch_topk": []} for n in NS for k in KS}
        info = {}
        for it in range(WARMUP + ROUNDS):
            for n in NS:
                for k in KS:
                    emb.timing()
                    emb.topk_device(n, rows, k, False)
                    emb.synchronize()
                    ms, launches, _ = emb.timing()
                    got_v, got_p = vals[:n * k].view(n, k), pos[:n * k].view(n, k)
                    emb.project_device(n, rows, False)
                    emb.synchronize()
                    ms_p = emb.timing()[0]
                    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    ref = torch.topk(logits[:n * rows].view(n, rows), k, dim=1)
                    b.record(); torch.cuda.synchronize()
                    if it >= WARMUP:
                        t = times[(n, k)]
                        t["topk"].append(ms); t["project"].append(ms_p); t["torch_topk"].append(a.elapsed_time(b))
                    info[(n, k)] = {"launches": int(launches), "torch_peak_bytes": int(torch.cuda.max_memory_allocated()),
                                    "values_equal": bool(torch.equal(got_v.view(torch.int32), ref.values.view(torch.int32))),
                                    "positions_equal": bool(torch.equal(got_p, ref.indices))}
                    del ref
        assert emb.bad_ids() == 0
        for (n, k), t in times.items():
            comp = [p + q for p, q in zip(t["project"], t["torch_topk"])]
            res = {"rows": rows, "dim": dim, "bitlevel": bitlevel, "n": n, "k": k,
                   "topk_ms_median": float(np.median(t["topk"])), "topk_ms_min": float(min(t["topk"])), "topk_ms_max": float(max(t["topk"])),
                   "project_ms_median": float(np.median(t["project"])), "torch_topk_ms_median": float(np.median(t["torch_topk"])),
                   "composition_ms_median": float(np.median(comp)), "topk_library_bytes": topk_bytes(rows, dim, n, k),
                   "composition_library_bytes": composition_bytes(rows, dim, n), **info[(n, k)]}
            res["time_vs_composition"] = res["topk_ms_median"] / res["composition_ms_median"]
            res["memory_vs_composition"] = res["topk_library_bytes"] / (res["composition_library_bytes"] + res["torch_peak_bytes"])
            out["cases"].append(res)
            print(json.dumps(res), flush=True)
        emb.close()
        del x_t, vals, pos, x_p, logits
json.dump(out, open(os.path.join("profiles", "embed_topk_bench.json"), "w"), indent=1)
