#!/usr/bin/env python3
"""Device time of the float-vector question (include/word2bits_eval.h, w2b_eval_vectors) on a bits and on a codes handle beside
the three-row top-k of an fp32 handle on the same shape, in one process: the text8 shape (19544 questions x 60238 rows x 200
dims, synthetic), random Gaussian query vectors, k = 10.  Every case is warmed up, then the cases are timed in turn,
`--repeats` rounds (so that a drift of the machine falls on all of them alike), HIP-event time from Evaluator.timing():
operands + scan + merge.  Each case is also given as a fraction of the f32 matrix bound that w2b_kernels_eval.hip derives,
78.6 T multiply-adds/s (questions x rows x size per launch; the codes path counts one multiply-add per column like the
others).  One JSON line on stdout (and in --out).

`--zero-queries` asks all-zero vectors instead: the launches, the loads and the matrix instructions are the same, but wx = 0,
no score is positive and the packed scans never enter their selection code -- what the scan costs without it.  Under
`rocprofv3 --kernel-trace --stats` (a run of its own) the same command gives the time per kernel.

    python tools/eval_vectors_bench.py --out profiles/eval_vectors_bench.json"""
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
from eval_codes_bench import write_packed as write_packed_codes  # noqa: E402

F32_MATRIX_BOUND = 78.6e12      # multiply-adds per second (w2b_kernels_eval.hip, "Bound")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=19544)
    ap.add_argument("--vocab", type=int, default=60238)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--zero-queries", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    x = rng.standard_normal((a.questions, a.dim)).astype(np.float32)
    if a.zero_queries:
        x[:] = 0
    b = rng.integers(0, a.vocab, (3, a.questions)).astype(np.int32)
    M = (rng.integers(0, 2, (a.vocab, a.dim)) * 2 - 1).astype(np.float32) / np.float32(3)
    res = {"shape": {"questions": a.questions, "vocab": a.vocab, "dim": a.dim, "k": a.k}, "warmup": a.warmup,
           "repeats": a.repeats, "zero_queries": a.zero_queries, "f32_matrix_bound_macs_per_s": F32_MATRIX_BOUND}
    with tempfile.TemporaryDirectory() as d:
        p1, p2, pf = os.path.join(d, "v1.w2bp"), os.path.join(d, "v2.w2bp"), os.path.join(d, "v.bin")
        write_packed(p1, random_packed(rng, a.vocab, a.dim), a.dim)
        write_packed_codes(p2, rng, a.vocab, a.dim)
        with open(pf, "wb") as f:
            f.write(b"%d %d\n" % M.shape)
            for i, row in enumerate(M):
                f.write(b"w%d " % i + row.tobytes() + b"\n")
        bits, codes, fp = w2b.Evaluator(p1, bits=True), w2b.Evaluator(p2, codes=True), w2b.Evaluator(pf, 0, 0, fused=True)
    cases = {"bits_vectors": (bits, lambda: bits.vectors(x, a.k)), "codes_vectors": (codes, lambda: codes.vectors(x, a.k)),
             "fp32_vectors": (fp, lambda: fp.vectors(x, a.k)), "fp32_topk": (fp, lambda: fp.topk(*b, a.k))}
    for ev, fn in cases.values():
        for _ in range(a.warmup):
            fn()
        ev.timing()
    ms = {name: [] for name in cases}
    for _ in range(a.repeats):
        for name, (ev, fn) in cases.items():
            fn()
            ms[name].append(ev.timing()[0])
    for ev in (bits, codes, fp):
        ev.close()
    macs = float(a.questions) * a.vocab * a.dim
    for name, runs in ms.items():
        med = statistics.median(runs)
        res[name] = {"median_ms": med, "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs,
                     "fraction_of_f32_matrix_bound": macs / (med * 1e-3) / F32_MATRIX_BOUND}
    for name in ("bits_vectors", "codes_vectors", "fp32_vectors"):
        res[name + "_vs_fp32_topk"] = res[name]["median_ms"] / res["fp32_topk"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
