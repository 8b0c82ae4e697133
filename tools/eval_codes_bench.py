#!/usr/bin/env python3
"""Device time of the codes-mode evaluator (include/word2bits_eval.h, "codes mode") beside the fp32 fused scan of the same
file, in one process and session: a seeded 2-bit model at 19544 questions x 60238 rows x `--dims` (200 and 400) -- fp32
fused top-1 and top-k as the yardstick, codes top-1 and top-k at k = 1, 10, 64.  Warm-up launches, then `--repeats` timed
ones, HIP-event time from Evaluator.timing().  One JSON line on stdout (and in --out).

    python tools/eval_codes_bench.py --out profiles/eval_codes_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/eval_codes_bench.py --dims 400 --only codes_top1 --repeats 3

The second form is the kernel-stats run of the top-1 case; it is a run of its own."""
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


def write_packed(path, rng, V, D):
    nb = (D + 63) // 64
    packed = rng.integers(0, 2 ** 64, (V, 2 * nb), dtype=np.uint64)
    packed[:, -2:] &= np.uint64((1 << (D - 64 * (nb - 1))) - 1)          # padding bits are zero in the file
    with open(path, "wb") as f:
        f.write(b"W2BP1 %d %d 2\n" % (V, D))
        f.write(b"".join(b"w%d\n" % i for i in range(V)))
        f.write(packed.astype("<u8").tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=19544)
    ap.add_argument("--vocab", type=int, default=60238)
    ap.add_argument("--dims", type=int, nargs="*", default=[200, 400])
    ap.add_argument("--k", type=int, nargs="*", default=[1, 10, 64])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", help="one case: fp32_top1, fp32_topk_<k>, codes_top1, codes_topk_<k>")
    ap.add_argument("--out")
    a = ap.parse_args()
    want = lambda name: a.only is None or a.only == name
    res = {"shape": {"questions": a.questions, "vocab": a.vocab, "vectors": "2bit"}, "warmup": a.warmup, "repeats": a.repeats}
    with tempfile.TemporaryDirectory() as d:
        for D in a.dims:
            rng = np.random.default_rng(D)
            pk = os.path.join(d, "v%d.w2bp" % D)
            write_packed(pk, rng, a.vocab, D)
            b = rng.integers(0, a.vocab, (3, a.questions)).astype(np.int32)
            r = {}
            for mode, ev in (("fp32", lambda: w2b.Evaluator(pk, 2, 0, fused=True)), ("codes", lambda: w2b.Evaluator(pk, codes=True))):
                names = ["%s_top1" % mode] + ["%s_topk_%d" % (mode, k) for k in a.k]
                if not any(want(n) for n in names):
                    continue
                e = ev()
                if want(names[0]):
                    r[names[0]] = timed(e, lambda: e.top1(*b), a.warmup, a.repeats)
                for k, n in zip(a.k, names[1:]):
                    if want(n):
                        r[n] = timed(e, lambda: e.topk(*b, k), a.warmup, a.repeats)
                e.close()
            for n in ["top1"] + ["topk_%d" % k for k in a.k]:
                if "fp32_" + n in r and "codes_" + n in r:
                    r["codes_vs_fp32_" + n] = r["codes_" + n]["median_ms"] / r["fp32_" + n]["median_ms"]
            res["dim_%d" % D] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
