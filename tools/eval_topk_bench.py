#!/usr/bin/env python3
"""Device time of the evaluator's top-1 scan and of the top-k scan + merge on the text8 shape (19544 questions x
60238 rows x 200 dims, 1-bit vectors, fused mode): warm-up launches, then `--repeats` timed ones, HIP-event time from
Evaluator.timing().  One JSON line on stdout (and in --out).

    python tools/eval_topk_bench.py --out profiles/eval_topk_bench.json
    W2B_LIB=<older libword2bits_hip.so> W2B_LIB_ALLOW_MISSING=1 python tools/eval_topk_bench.py --top1-only

The second form measures the top-1 scan of another build of the library (an A/B against the parent commit has to
run on the same machine in the same session)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import word2bits_amd as w2b  # noqa: E402


def timed(ev, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ev.timing()
    ms = []
    for _ in range(repeats):
        fn()
        ms.append(ev.timing()[0])
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=19544)
    ap.add_argument("--vocab", type=int, default=60238)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--k", type=int, nargs="*", default=[1, 10, 64])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--top1-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    M = (rng.integers(0, 2, (a.vocab, a.dim)) * 2 - 1).astype(np.float32) / np.float32(3)
    b = rng.integers(0, a.vocab, (3, a.questions)).astype(np.int32)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "v.bin")
        with open(path, "wb") as f:
            f.write(b"%d %d\n" % M.shape)
            for i, row in enumerate(M):
                f.write(b"w%d " % i + row.tobytes() + b"\n")
        ev = w2b.Evaluator(path, 0, 0, fused=True)
    res = {"shape": {"questions": a.questions, "vocab": a.vocab, "dim": a.dim, "vectors": "1bit", "mode": "fused"},
           "warmup": a.warmup, "repeats": a.repeats, "library": os.path.basename(os.path.dirname(w2b._lib.LIB_PATH)),
           "top1": timed(ev, lambda: ev.top1(*b), a.warmup, a.repeats)}
    if not a.top1_only:
        for k in a.k:
            res["topk_%d" % k] = timed(ev, lambda: ev.topk(*b, k), a.warmup, a.repeats)
            res["topk_%d" % k]["vs_top1"] = res["topk_%d" % k]["median_ms"] / res["top1"]["median_ms"]
    ev.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
