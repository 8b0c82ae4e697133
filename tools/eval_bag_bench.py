#!/usr/bin/env python3
"""Device time of the bag question (include/word2bits_eval.h, w2b_eval_bag) on both packed modes, beside a yardstick of the
same handle in the same process: the text8 shape (19544 bags x 60238 rows x 200 dims, synthetic), bags of 3 and of 32 ids,
k = 1 and k = 10.  Yardsticks: on a bits handle w2b_eval_combine with the same three rows, all +, which returns the same
lists; on a codes handle w2b_eval_topk.  Every case is warmed up, then the cases are timed in turn, `--repeats` rounds (so
that a drift of the machine falls on all of them alike), HIP-event time from Evaluator.timing(): operands + scan + merge.
One JSON line on stdout (and in --out).

    python tools/eval_bag_bench.py --out profiles/eval_bag_bench.json"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import word2bits_amd as w2b  # noqa: E402
import eval_bits_bench  # noqa: E402
import eval_codes_bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=19544)
    ap.add_argument("--vocab", type=int, default=60238)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--lengths", type=int, nargs="*", default=[3, 32])
    ap.add_argument("--k", type=int, nargs="*", default=[1, 10])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    rows = {m: rng.integers(0, a.vocab, (a.questions, m)).astype(np.int32) for m in sorted(set(a.lengths) | {3})}
    offsets = {m: np.arange(a.questions + 1, dtype=np.int64) * m for m in rows}
    three, plus = rows[3], np.ones((a.questions, 3), np.int8)
    res = {"shape": {"questions": a.questions, "vocab": a.vocab, "dim": a.dim, "vectors": "synthetic"},
           "lengths": a.lengths, "warmup": a.warmup, "repeats": a.repeats}
    with tempfile.TemporaryDirectory() as d:
        p1, p2 = os.path.join(d, "v1.w2bp"), os.path.join(d, "v2.w2bp")
        eval_bits_bench.write_packed(p1, eval_bits_bench.random_packed(rng, a.vocab, a.dim), a.dim)
        eval_codes_bench.write_packed(p2, rng, a.vocab, a.dim)
        evs = {"bits": w2b.Evaluator(p1, bits=True), "codes": w2b.Evaluator(p2, codes=True)}
        cases = {}                                           # name -> (handle, call)
        for k in a.k:
            cases["bits_combine3_%d" % k] = ("bits", lambda k=k: evs["bits"].combine(three, plus, k))
            cases["codes_topk_%d" % k] = ("codes", lambda k=k: evs["codes"].topk(three[:, 0], three[:, 1], three[:, 2], k))
            for mode in evs:
                for m in a.lengths:
                    cases["%s_bag%d_%d" % (mode, m, k)] = (mode, lambda k=k, m=m, mode=mode: evs[mode].bag(rows[m].ravel(), offsets[m], k))
        for k in a.k:                                        # same answers, or the times compare nothing
            r0, d0 = cases["bits_combine3_%d" % k][1]()
            r1, d1 = evs["bits"].bag(three.ravel(), offsets[3], k)
            assert np.array_equal(r0, r1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
        for _, fn in cases.values():
            for _ in range(a.warmup):
                fn()
        for ev in evs.values():
            ev.timing()
        ms = {name: [] for name in cases}
        for _ in range(a.repeats):
            for name, (mode, fn) in cases.items():
                fn()
                ms[name].append(evs[mode].timing()[0])
        for ev in evs.values():
            ev.close()
    for name, runs in ms.items():
        res[name] = {"median_ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}
    for k in a.k:
        for m in a.lengths:
            res["bits_bag%d_%d_vs_combine3_%d" % (m, k, k)] = res["bits_bag%d_%d" % (m, k)]["median_ms"] / res["bits_combine3_%d" % k]["median_ms"]
            res["codes_bag%d_%d_vs_topk_%d" % (m, k, k)] = res["codes_bag%d_%d" % (m, k)]["median_ms"] / res["codes_topk_%d" % k]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
