#!/usr/bin/env python3
"""Device time of the word classes (include/word2bits_eval.h, w2b_eval_classes) on both packed modes, at word2vec's demo
shape: 60238 rows x 200 dims (synthetic, random: k-means does not converge early on it), K = 500, 10 iterations asked for;
iters_run is reported.  Per iteration the time of the assign scan and of the sums pass (HIP-event pairs around each,
Evaluator.classes_timing()), and the assign's share of the 157.3 TFLOP/s f32 matrix peak on PADDED multiply-adds (classes to
64, rows to 256, columns to 8: what the matrix cores are given).  For orientation, in the same process and on the same
handle: vectors(x, k=1) with 512 random questions -- about the same number of multiply-adds through the merged scan whose
operand roles the assign swaps.  Every case is warmed up, then the cases are timed in turn, `--repeats` rounds (so that a drift
of the machine falls on all of them alike).  Nothing is gated.  One JSON line on stdout (and in --out).

    python tools/eval_classes_bench.py --out profiles/eval_classes_bench.json
    python tools/eval_classes_bench.py --vocab 1000000 --dim 200 --out profiles/eval_classes_bench_1m.json"""
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

F32_MATRIX_PEAK = 157.3e12


def stats(runs):
    return {"median_ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=60238)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--classes", type=int, default=500)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--questions", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    x = rng.standard_normal((a.questions, a.dim)).astype(np.float32)
    up = lambda n, m: (n + m - 1) // m * m
    padded = float(up(a.classes, 64)) * up(a.vocab, 256) * up(a.dim, 8)
    res = {"shape": {"vocab": a.vocab, "dim": a.dim, "classes": a.classes, "iters": a.iters, "questions": a.questions},
           "warmup": a.warmup, "repeats": a.repeats, "padded_macs_per_iteration": padded}
    with tempfile.TemporaryDirectory() as d:
        for mode in ("bits", "codes"):
            pk = os.path.join(d, mode + ".w2bp")
            if mode == "bits":
                write_packed_bits(pk, random_packed(rng, a.vocab, a.dim), a.dim)
            else:
                write_packed_codes(pk, rng, a.vocab, a.dim)
            ev = w2b.Evaluator(pk, bits=mode == "bits", codes=mode == "codes")
            for _ in range(a.warmup):
                ev.classes(a.classes, a.iters)
                ev.vectors(x, 1)
            ev.timing()
            total, assign, sums, vec, iters_run = [], [], [], [], []
            for _ in range(a.repeats):
                it = ev.classes(a.classes, a.iters, details=True)[4]
                total.append(ev.timing()[0])
                t = ev.classes_timing()
                assign.append(t[0] / max(it, 1))
                sums.append(t[1] / (it + 1))                    # one sums pass ahead of the first iteration
                iters_run.append(it)
                ev.vectors(x, 1)
                vec.append(ev.timing()[0])
            ev.close()
            out = {"iters_run": iters_run, "classes_total": stats(total), "assign_per_iteration": stats(assign),
                   "sums_per_pass": stats(sums), "vectors_512_k1": stats(vec)}
            out["assign_share_of_f32_matrix_peak"] = 2.0 * padded / (out["assign_per_iteration"]["median_ms"] * 1e-3) / F32_MATRIX_PEAK
            out["assign_vs_vectors"] = out["assign_per_iteration"]["median_ms"] / out["vectors_512_k1"]["median_ms"]
            res[mode] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
