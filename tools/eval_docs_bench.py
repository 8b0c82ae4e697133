#!/usr/bin/env python3
"""Device time of the document question (include/word2bits_eval.h, w2b_eval_docs) on both packed modes: 60238 rows x 200 dims
(synthetic, random), a corpus of 1,000,000 documents with lengths uniform in 5..35 and uniformly random ids, 64 queries of 20
ids, k = 10, symmetric = 1.  Per mode: the total device time of a call (Evaluator.timing()), its table phase and its walk phase
(Evaluator.docs_timing()), and the table bytes per second that the walk reads -- every (query, document position) pair is one
read of the query's slice of a table row (its columns x 4 bytes), plus 4 bytes of row maximum for the other direction.  That rate
is to be held against the gather rates that a table of this size (larger than the 256 MiB Infinity Cache, with hot lines in L2)
is served at; the share is a measurement of the run, not a target.  For context only: the host twin's time for one query on
1/100 of the corpus, scaled to all queries and the whole corpus.  Nothing is gated.

Each mode is measured in a child process of its own under `timeout`; the first one that fails ends the run.  One JSON line on
stdout (and in --out).

    python tools/eval_docs_bench.py --out profiles/eval_docs_bench.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import word2bits_amd as w2b  # noqa: E402
from word2bits_amd import _lib  # noqa: E402
from eval_bits_bench import random_packed, write_packed as write_packed_bits  # noqa: E402
from eval_codes_bench import write_packed as write_packed_codes  # noqa: E402


def stats(runs):
    return {"median_ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}


def twin_ms(packed, dim, bitlevel, ids, offsets, q):
    """the host twin's time for ONE query against the given documents"""
    n = len(offsets) - 1
    sc = np.empty(n, np.float32)
    t0 = time.perf_counter()
    _lib.check(_lib.lib().w2b_docs_scores_host(packed.ctypes.data_as(_lib.u64p), packed.shape[0], dim, bitlevel, int(offsets[-1]),
                                               ids.ctypes.data_as(_lib.i32p), n, offsets.ctypes.data_as(_lib.i64p), len(q),
                                               q.ctypes.data_as(_lib.i32p), 1, None, sc.ctypes.data_as(_lib.f32p)))
    return (time.perf_counter() - t0) * 1e3


def one_mode(a, mode):
    rng = np.random.default_rng(1)
    lens = rng.integers(a.min_len, a.max_len + 1, a.docs)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = rng.integers(0, a.vocab, int(offsets[-1])).astype(np.int32)
    qids = rng.integers(0, a.vocab, a.queries * a.query_len).astype(np.int32)
    qoff = (np.arange(a.queries + 1) * a.query_len).astype(np.int64)
    with tempfile.TemporaryDirectory() as d:
        pk = os.path.join(d, mode + ".w2bp")
        if mode == "bits":
            write_packed_bits(pk, random_packed(rng, a.vocab, a.dim), a.dim)
        else:
            write_packed_codes(pk, rng, a.vocab, a.dim)
        ev = w2b.Evaluator(pk, bits=mode == "bits", codes=mode == "codes")
    ev.set_docs(ids, offsets)
    for _ in range(a.warmup):
        ev.docs(qids, qoff, a.k)
    ev.timing()
    total, table, walk, chunks = [], [], [], []
    for _ in range(a.repeats):
        ev.docs(qids, qoff, a.k)
        ms, launches, _ = ev.timing()
        t = ev.docs_timing()
        total.append(ms)
        table.append(t[0])
        walk.append(t[1])
        chunks.append(launches)
    packed = ev.bits() if mode == "bits" else ev.codes()
    ev.close()
    width = (a.query_len + 15) // 16 * 16
    walk_bytes = float(a.queries) * float(offsets[-1]) * (4.0 * width + 4.0)
    out = {"total": stats(total), "table_phase": stats(table), "walk_phase": stats(walk), "chunks_per_call": chunks,
           "table_bytes": 4.0 * a.vocab * (width + 1) * a.queries, "walk_table_bytes_read": walk_bytes}
    out["walk_table_bytes_per_s"] = walk_bytes / (out["walk_phase"]["median_ms"] * 1e-3)
    n100 = max(a.docs // 100, 1)
    one = twin_ms(packed, a.dim, 1 if mode == "bits" else 2, ids, offsets[:n100 + 1], qids[:a.query_len])
    out["host_twin_scaled_ms"] = one * (a.docs / n100) * a.queries
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=60238)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--min-len", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=35)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--query-len", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds that one mode's child process may take")
    ap.add_argument("--mode", choices=["bits", "codes"], help="(internal) measure this mode in this process")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode:
        print(json.dumps(one_mode(a, a.mode)))
        return 0
    res = {"shape": {"vocab": a.vocab, "dim": a.dim, "docs": a.docs, "doc_len": [a.min_len, a.max_len], "queries": a.queries,
                     "query_len": a.query_len, "k": a.k, "symmetric": 1}, "warmup": a.warmup, "repeats": a.repeats}
    passed = [x for x in sys.argv[1:]]
    for mode in ("bits", "codes"):
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--mode", mode] + passed,
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print("eval_docs_bench: mode %s ended with status %d; stopping" % (mode, r.returncode), file=sys.stderr)
            return r.returncode
        res[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
