#!/usr/bin/env python3
"""Device time of the bits-mode evaluator (include/word2bits_eval.h, "bits mode") beside the fp32 scan of the same tree,
in one process and session: the text8 shape (19544 questions x 60238 rows x 200 dims, 1-bit) -- fp32 fused top-1 and
top-k (k = 10) as the yardstick, bits top-1 and top-k at k = 1, 10, 64 -- and the large case (1 000 000 rows x 1000
dims, `--big-questions` questions).  Warm-up launches, then `--repeats` timed ones, HIP-event time from
Evaluator.timing().  One JSON line on stdout (and in --out).

    python tools/eval_bits_bench.py --out profiles/eval_bits_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/eval_bits_bench.py --only bits_topk_10 --repeats 3

The second form is the kernel-stats run of the k = 10 case; it is a run of its own."""
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


def random_packed(rng, V, D):
    wpr = (D + 63) // 64
    packed = rng.integers(0, 2 ** 64, (V, wpr), dtype=np.uint64)
    packed[:, -1] &= np.uint64((1 << (D - 64 * (wpr - 1))) - 1)          # padding bits are zero in the file
    return packed


def write_packed(path, packed, D):
    with open(path, "wb") as f:
        f.write(b"W2BP1 %d %d 1\n" % (packed.shape[0], D))
        f.write(b"".join(b"w%d\n" % i for i in range(packed.shape[0])))
        f.write(packed.astype("<u8").tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=19544)
    ap.add_argument("--vocab", type=int, default=60238)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--k", type=int, nargs="*", default=[1, 10, 64])
    ap.add_argument("--big-vocab", type=int, default=1_000_000)
    ap.add_argument("--big-dim", type=int, default=1000)
    ap.add_argument("--big-questions", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", help="one case: fp32_top1, fp32_topk_10, bits_top1, bits_topk_<k>, big")
    ap.add_argument("--out")
    a = ap.parse_args()
    want = lambda name: a.only is None or a.only == name
    rng = np.random.default_rng(1)
    packed = random_packed(rng, a.vocab, a.dim)
    b = rng.integers(0, a.vocab, (3, a.questions)).astype(np.int32)
    res = {"shape": {"questions": a.questions, "vocab": a.vocab, "dim": a.dim, "vectors": "1bit"},
           "warmup": a.warmup, "repeats": a.repeats}
    with tempfile.TemporaryDirectory() as d:
        pk = os.path.join(d, "v.w2bp")
        write_packed(pk, packed, a.dim)
        if want("fp32_top1") or want("fp32_topk_10"):
            ev = w2b.Evaluator(pk, 0, 0, fused=True)                     # the same model through the fp32 path
            if want("fp32_top1"):
                res["fp32_top1"] = timed(ev, lambda: ev.top1(*b), a.warmup, a.repeats)
            if want("fp32_topk_10"):
                res["fp32_topk_10"] = timed(ev, lambda: ev.topk(*b, 10), a.warmup, a.repeats)
            ev.close()
        ev = w2b.Evaluator(pk, bits=True)
        if want("bits_top1"):
            res["bits_top1"] = timed(ev, lambda: ev.top1(*b), a.warmup, a.repeats)
        for k in a.k:
            if want("bits_topk_%d" % k):
                res["bits_topk_%d" % k] = timed(ev, lambda: ev.topk(*b, k), a.warmup, a.repeats)
        ev.close()
        if "fp32_top1" in res and "bits_top1" in res:
            res["bits_top1_vs_fp32_top1"] = res["bits_top1"]["median_ms"] / res["fp32_top1"]["median_ms"]
        if "fp32_topk_10" in res and "bits_topk_10" in res:
            res["bits_topk_10_vs_fp32_topk_10"] = res["bits_topk_10"]["median_ms"] / res["fp32_topk_10"]["median_ms"]
        if want("big") and a.big_vocab > 0:
            big = random_packed(rng, a.big_vocab, a.big_dim)
            bp = os.path.join(d, "big.w2bp")
            write_packed(bp, big, a.big_dim)
            del big
            bq = rng.integers(0, a.big_vocab, (3, a.big_questions)).astype(np.int32)
            ev = w2b.Evaluator(bp, bits=True)
            res["big"] = {"shape": {"questions": a.big_questions, "vocab": a.big_vocab, "dim": a.big_dim},
                          "bits_top1": timed(ev, lambda: ev.top1(*bq), a.warmup, a.repeats),
                          "bits_topk_10": timed(ev, lambda: ev.topk(*bq, 10), a.warmup, a.repeats)}
            ev.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
