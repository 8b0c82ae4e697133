#!/usr/bin/env python3
"""Device time of the signed multi-word question on a bits handle (include/word2bits_eval.h, w2b_eval_combine) beside the
three-row top-k of the same handle, in one process: the text8 shape (19544 questions x 60238 rows x 200 dims, 1-bit,
synthetic) -- topk(b1, b2, b3, k) and combine(+b2, -b1, +b3, k), which return the same lists, at k = 1 and k = 10, and a
7-term combine.  Every case is warmed up, then the cases are timed in turn, `--repeats` rounds (so that a drift of the
machine falls on all of them alike), HIP-event time from Evaluator.timing(): planes + scan + merge.  One JSON line on
stdout (and in --out).

    python tools/eval_combine_bench.py --out profiles/eval_combine_bench.json"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import word2bits_amd as w2b  # noqa: E402
from eval_bits_bench import random_packed, write_packed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=19544)
    ap.add_argument("--vocab", type=int, default=60238)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--k", type=int, nargs="*", default=[1, 10])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    b = rng.integers(0, a.vocab, (3, a.questions)).astype(np.int32)
    three, plus_minus_plus = np.stack([b[1], b[0], b[2]], 1), np.tile(np.array([1, -1, 1], np.int8), (a.questions, 1))
    seven = rng.integers(0, a.vocab, (a.questions, 7)).astype(np.int32)
    seven_signs = np.tile(np.array([1, -1, 1, 1, -1, 1, -1], np.int8), (a.questions, 1))
    res = {"shape": {"questions": a.questions, "vocab": a.vocab, "dim": a.dim, "vectors": "1bit"},
           "warmup": a.warmup, "repeats": a.repeats}
    with tempfile.TemporaryDirectory() as d:
        pk = os.path.join(d, "v.w2bp")
        write_packed(pk, random_packed(rng, a.vocab, a.dim), a.dim)
        ev = w2b.Evaluator(pk, bits=True)
        cases = {}
        for k in a.k:
            cases["topk_%d" % k] = lambda k=k: ev.topk(*b, k)
            cases["combine3_%d" % k] = lambda k=k: ev.combine(three, plus_minus_plus, k)
            cases["combine7_%d" % k] = lambda k=k: ev.combine(seven, seven_signs, k)
        for k in a.k:                                        # same answers, or the times compare nothing
            r0, d0 = cases["topk_%d" % k]()
            r1, d1 = cases["combine3_%d" % k]()
            assert np.array_equal(r0, r1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
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
    for name, runs in ms.items():
        res[name] = {"median_ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}
    for k in a.k:
        res["combine3_%d_vs_topk_%d" % (k, k)] = res["combine3_%d" % k]["median_ms"] / res["topk_%d" % k]["median_ms"]
        res["combine7_%d_vs_topk_%d" % (k, k)] = res["combine7_%d" % k]["median_ms"] / res["topk_%d" % k]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
