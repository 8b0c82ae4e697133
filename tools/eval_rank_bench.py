#!/usr/bin/env python3
"""Device time of the rank question (include/word2bits_eval.h, w2b_eval_rank) beside the list scans of the same handle, in
one process, on both packed modes: the evaluator benchmark's shape (19544 questions x 60238 rows x 200 dims, synthetic) --
rank(b1, b2, b3, target) with random targets, top1(b1, b2, b3) (the scan whose shape the rank kernels share), and
topk(b1, b2, b3, k) at k = 1 and k = 64, all on the same questions.  Every case is warmed up, then the cases are timed in
turn, `--repeats` rounds (so that a drift of the machine falls on all of them alike), HIP-event time from Evaluator.timing():
operands / planes + target scores + scan (+ merge).  One JSON line on stdout (and in --out).

    python tools/eval_rank_bench.py --out profiles/eval_rank_bench.json"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import word2bits_amd as w2b  # noqa: E402
from eval_bits_bench import random_packed, write_packed as write_packed_bits  # noqa: E402
from eval_codes_bench import write_packed as write_packed_codes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=19544)
    ap.add_argument("--vocab", type=int, default=60238)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--k", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    b = rng.integers(0, a.vocab, (3, a.questions)).astype(np.int32)
    g = rng.integers(0, a.vocab, a.questions).astype(np.int32)
    res = {"shape": {"questions": a.questions, "vocab": a.vocab, "dim": a.dim}, "warmup": a.warmup, "repeats": a.repeats}
    with tempfile.TemporaryDirectory() as d:
        for mode in ("bits", "codes"):
            pk = os.path.join(d, mode + ".w2bp")
            if mode == "bits":
                write_packed_bits(pk, random_packed(rng, a.vocab, a.dim), a.dim)
            else:
                write_packed_codes(pk, rng, a.vocab, a.dim)
            ev = w2b.Evaluator(pk, bits=mode == "bits", codes=mode == "codes")
            ranks = []
            cases = {"rank": lambda: ranks.append(ev.rank(*b, g)), "top1": lambda: ev.top1(*b)}
            for k in a.k:
                cases["topk_%d" % k] = lambda k=k: ev.topk(*b, k)
            for fn in cases.values():
                for _ in range(a.warmup):
                    fn()
            ev.timing()
            ms = {name: [] for name in cases}
            for _ in range(a.repeats):
                for name, fn in cases.items():
                    fn()
                    ms[name].append(ev.timing()[0])
            ev.close()
            out = {}
            for name, runs in ms.items():
                out[name] = {"median_ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}
            out["rank_vs_top1"] = out["rank"]["median_ms"] / out["top1"]["median_ms"]
            out["rank_minus_top1_ms"] = out["rank"]["median_ms"] - out["top1"]["median_ms"]
            out["top1_spread_ms"] = out["top1"]["max_ms"] - out["top1"]["min_ms"]
            for k in a.k:
                out["rank_vs_topk_%d" % k] = out["rank"]["median_ms"] / out["topk_%d" % k]["median_ms"]
            r = ranks[-1]
            out["ranked_targets"] = int((r > 0).sum())
            out["mean_rank_of_ranked"] = float(r[r > 0].mean()) if (r > 0).any() else 0.0
            assert all(np.array_equal(x, r) for x in ranks)     # every repeat gives the same ranks
            res[mode] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
