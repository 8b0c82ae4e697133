#!/usr/bin/env python3
"""Device time of the pair question (include/word2bits_eval.h, w2b_eval_pairs) in one process on one GPU: synthetic 1-bit and
2-bit tables of 60 238 x 200 and 400 000 x 800, two workloads of 1 M pairs with Zipf-distributed ids -- one-word pairs, and
pairs of 20-word bags -- and beside each the pooling alone, done by the existing bag kernel: PackedEmbedding.bag(..., "sum")
on the same 2 M bags (in slices, so that its float32 output stays small on the host; it writes 2 M x dim floats that the pair
kernel never materialises).  HIP-event time from Evaluator.timing() and PackedEmbedding.timing().  Every case is warmed up,
then the cases are timed in turn, `--repeats` rounds (so that a drift of the machine falls on all of them alike); medians.
`bytes` = n_ids x words per row x 8 + pairs x 24: the packed words pooled and the three integers written.  One JSON line on
stdout (and in --out).

    python tools/eval_pairs_bench.py --out profiles/eval_pairs_bench.json"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_packed(path, packed, dim, bitlevel):
    """the .w2bp format of include/word2bits_corpus.h"""
    with open(path, "wb") as f:
        f.write(b"W2BP1 %d %d %d\n" % (packed.shape[0], dim, bitlevel))
        f.write(b"".join(b"w%d\n" % i for i in range(packed.shape[0])))
        f.write(np.ascontiguousarray(packed, "<u8").tobytes())
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["60238x200", "400000x800"])
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--bag", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pool-slice", type=int, default=250_000, help="bags per PackedEmbedding.bag call")
    ap.add_argument("--out")
    a = ap.parse_args()
    import word2bits_amd as w2b
    rng = np.random.default_rng(1)
    res = {"pairs": a.pairs, "bag": a.bag, "ids_distribution": "zipf(1)", "warmup": a.warmup, "repeats": a.repeats, "cases": {}}
    tmp = tempfile.mkdtemp(prefix="eval_pairs_bench_")
    for shape in a.shapes:
        rows, dim = (int(x) for x in shape.split("x"))
        cdf = np.cumsum(1.0 / np.arange(1, rows + 1))
        cdf /= cdf[-1]
        zipf = lambda n: np.minimum(np.searchsorted(cdf, rng.random(n)), rows - 1).astype(np.int32)   # row = frequency rank
        loads = {"one_word": 1, "bags_of_%d" % a.bag: a.bag}
        ids = {name: zipf(2 * a.pairs * m) for name, m in loads.items()}
        offsets = {name: np.arange(2 * a.pairs + 1, dtype=np.int64) * m for name, m in loads.items()}
        for bitlevel in (1, 2):
            wpr = w2b.packed_words_per_row(dim, bitlevel)
            packed = rng.integers(0, 2 ** 64, (rows, wpr), dtype=np.uint64)
            if dim % 64:
                packed[:, -bitlevel:] &= np.uint64((1 << (dim % 64)) - 1)
            path = write_packed(os.path.join(tmp, "m.w2bp"), packed, dim, bitlevel)
            ev = w2b.Evaluator(path, bits=bitlevel == 1, codes=bitlevel == 2)
            emb = w2b.PackedEmbedding(packed=packed, dim=dim, bitlevel=bitlevel)
            os.remove(path)

            def pairs_ms(name):
                ev.pairs(ids[name], offsets[name])
                ms, launches, macs = ev.timing()
                assert macs == float(len(ids[name])) * dim
                return ms

            def pool_ms(name):
                m, total = loads[name], 0.0
                for b0 in range(0, 2 * a.pairs, a.pool_slice):
                    b1 = min(2 * a.pairs, b0 + a.pool_slice)
                    emb.bag(ids[name][b0 * m:b1 * m], offsets[name][b0:b1 + 1] - b0 * m, "sum")
                    total += emb.timing()[0]
                return total

            # the same answers on a sample, or the times compare nothing: the cosine of the pooled float rows
            for name, m in loads.items():
                n = 1000
                score = ev.pairs(ids[name][:2 * n * m], offsets[name][:2 * n + 1])
                pooled = emb.bag(ids[name][:2 * n * m], offsets[name][:2 * n + 1], "sum").astype(np.float64)
                A, B = pooled[0::2], pooled[1::2]
                want = (A * B).sum(1) / np.sqrt((A * A).sum(1) * (B * B).sum(1))
                assert np.allclose(score, want, rtol=0, atol=1e-5), name
            ev.timing()
            emb.timing()
            cases = [(fn, name) for name in loads for fn in (pairs_ms, pool_ms)]
            for fn, name in cases:
                for _ in range(a.warmup):
                    fn(name)
            ev.timing()
            emb.timing()
            runs = {(fn.__name__, name): [] for fn, name in cases}
            for _ in range(a.repeats):
                for fn, name in cases:
                    runs[(fn.__name__, name)].append(fn(name))
            entry = {"rows": rows, "dim": dim, "bitlevel": bitlevel, "packed_bytes": int(packed.nbytes)}
            for name, m in loads.items():
                p, q = runs[("pairs_ms", name)], runs[("pool_ms", name)]
                nbytes = len(ids[name]) * wpr * 8 + a.pairs * 24
                pm, qm = statistics.median(p), statistics.median(q)
                entry[name] = {"n_ids": int(len(ids[name])), "pairs_median_ms": pm, "pairs_min_ms": min(p), "pairs_max_ms": max(p),
                               "bytes": int(nbytes), "gbs": nbytes / (pm * 1e-3) / 1e9, "pooling_only_median_ms": qm,
                               "pooling_only_min_ms": min(q), "pooling_only_max_ms": max(q), "time_vs_pooling_only": pm / qm}
            res["cases"]["%s_bitlevel%d" % (shape, bitlevel)] = entry
            print("%s bitlevel %d done" % (shape, bitlevel), file=sys.stderr, flush=True)
            ev.close()
            emb.close()
    os.rmdir(tmp)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
