#!/usr/bin/env python3
"""Device milliseconds of one replica exchange through the library's own pipeline (w2b_sync_replicas on a communicator of
size 1, w2b_sync_stats) at the headline shape: V = 400 K, size 800, ten chunks of 64 Mi floats.  Prints one JSON line.
W2B_LIB selects the library, as everywhere (word2bits_amd/_lib.py)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=400_000)
    ap.add_argument("--dim", type=int, default=800)
    ap.add_argument("--mode", type=int, default=2)
    ap.add_argument("--exchanges", type=int, default=8)
    args = ap.parse_args()
    import numpy as np
    import word2bits_amd as w2b
    V = args.vocab
    t = w2b.Trainer(V, args.dim, 8, 24, 1, num_threads=1, iter=1, sample=0.0, compute_loss=False)
    t.init_net()
    counts = np.concatenate([[1], np.maximum(1e8 / np.arange(1, V), 5)]).astype(np.int64)      # Zipf(1), sorted by count
    t.set_vocab_counts(counts, 1_000_000)
    t.comm_init(1, 0, w2b.comm_unique_id())
    t.sync_replicas(args.mode)                                  # warm-up: RCCL's first collective, first use of the kernels
    t.sync_stats()
    for _ in range(args.exchanges):
        t.sync_replicas(args.mode)
    n, ms = t.sync_stats()
    t.close()
    print(json.dumps({"metric": "exchange_device_ms", "value": ms / n, "unit": "ms", "exchanges": n, "mode": args.mode,
                      "floats": 2 * V * args.dim, "chunks": -(-2 * V * args.dim // (64 << 20)), "lib": w2b.LIB_PATH}))


if __name__ == "__main__":
    main()
