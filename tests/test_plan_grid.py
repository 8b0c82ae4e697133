"""The launch policy (word2bits_amd/csrc/w2b_plan.cpp) over a grid of configurations, without a GPU: w2b_plan_rows is pure
host arithmetic, and tests/golden/plan_grid.json records what the library decided for every case of the grid BEFORE the
policy moved into a translation unit of its own.  A refactoring of the policy must reproduce every one of them.

The cases are generated from a fixed seed (they are not stored); the recording holds the nine integers of w2b_row_plan per
case, in the order of _lib.RowPlan._fields_.  To record again -- only ever with a library whose decisions are the ones to
keep, e.g. the build of the parent commit --:  W2B_LIB=/path/to/libword2bits_hip.so W2B_RECORD_PLAN_GRID=1 python -m pytest
tests/test_plan_grid.py
"""
import ctypes as C
import json
import os

import numpy as np

from word2bits_amd import _lib
from w2b_testlib import GOLDEN

PLAN_GRID_JSON = os.path.join(GOLDEN, "plan_grid.json")
FIELDS = [k for k, _ in _lib.RowPlan._fields_]
CASES = 4400


def _vocabularies():
    def zipf(V, top, eos):
        cn = np.maximum((top / np.arange(1, V + 1)).astype(np.int64), 5)
        cn[0] = eos                                                             # "</s>"
        return cn
    return {"zipf400k": zipf(400_000, 7.4e6, 100_000), "zipf70k": zipf(70_000, 1.45e6, 17_000),
            "flat300": np.full(2129, 300, np.int64), "flat30000": np.full(2129, 30_000, np.int64),
            "three": np.array([10, 7, 3], np.int64)}


WORKERS = [1, 2, 16, 17, 64, 128, 256, 257, 640, 641, 767, 768, 1024, 2048]   # around every threshold at 256 CUs, and between
NUM_CUS = [64, 256, 304]
# both sides of 512 (automatic row-group kernel), 1024 (widest row with atomic adds), 4096 / 1024 columns (the wide form), and
# rows that are not a multiple of four floats
DIMS = [100, 200, 201, 300, 400, 508, 512, 516, 800, 1020, 1023, 1024, 1025, 1028, 2048, 4096, 4100]
SAMPLES = [0.0, 1e-3, 1e-4]
TRAIN_WORDS = [0.0, 0.1, 1.0, 10.0]                                            # x the sum of the counts
# every knob of w2b_tuning that the row rules read, off its default
TUNE = {"hot_rows_u": [0, 5, 40], "hot_rows_v": [0, 4, 40], "hot_period": [1, 8, 64], "hot_cap": [0, 8, 32],
        "force_row_desc": [1], "mem_mode": [0, 1], "atomic_rank": [0, 100, 10 ** 6], "atomic_cap": [10, 1000],
        "atomic_rank_u": [-1, 50, 10 ** 6], "fresh_rank_u": [-1, 10], "refresh_rows_u": [-1, 8, 64],
        "concurrent_workers": [1, 7, 100]}


def _cases():
    """Three strata, 2 : 2 : 1 -- a uniform draw over the lists above, one restricted to what the row-group kernel accepts, one
    to the small flat vocabularies with coherent rows, where target rows get lossless adds (a uniform draw alone gives 4 %
    row-group cases, 1 % refreshed rows and 6 % lossless target rows: a grid of zeros would hide differences)."""
    state = [0x9E3779B97F4A7C15]

    def below(n):                                                               # a 64-bit LCG of our own: the same cases everywhere
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (state[0] >> 33) % n

    def pick(seq):
        return seq[below(len(seq))]
    knobs = sorted(TUNE)
    for i in range(CASES):
        groups, flat = i % 5 in (1, 3), i % 5 == 2
        c = {"vocab": pick(["zipf400k", "zipf70k"] if groups else ["flat300", "flat30000", "three"] if flat
                           else ["zipf400k", "zipf70k", "flat300", "flat30000", "three"]),
             "workers": pick([16, 17, 64, 128, 128, 256, 256, 256] if groups else WORKERS),   # (refreshed rows: from 40 workers on)
             "num_cus": pick(NUM_CUS[1:] if groups else NUM_CUS),              # (64 CUs: 256 workers are a full device)
             "dim": pick([d for d in DIMS if d <= 512 and d % 4 == 0] if groups else DIMS),
             "window": 1 + below(16 if groups else 17),
             "negative": 5 + below(20 if groups else 26),
             "sample": pick(SAMPLES),
             "plain_worker_kernel": pick([0, 0, 3, 3, 1, 2]) if groups else below(4),
             "relaxed_coherence": 0 if groups or flat else int(below(4) == 0),
             "exact_reduction": 0 if groups or flat else int(below(4) == 0),
             "total_threads": int(below(4 if groups else 2) == 0) * 8,          # x workers
             "train_words": pick(TRAIN_WORDS[2:] if groups else TRAIN_WORDS),
             "tune": None}
        if below(5) >= (3 if groups else 2):                                    # 3 (2) of 5 cases: one knob off its default
            k = pick(knobs)
            c["tune"] = (k, pick(TUNE[k]))
        yield c


def _plan(L, vocab, c):
    cn = vocab[c["vocab"]]
    cfg = _lib.Config()
    cfg.vocab_size, cfg.train_words, cfg.iter = len(cn), int(c["train_words"] * int(cn.sum())), 1
    cfg.layer1_size, cfg.window, cfg.negative, cfg.bitlevel, cfg.num_threads = c["dim"], c["window"], c["negative"], 1, c["workers"]
    cfg.alpha, cfg.sample = 0.05, c["sample"]
    cfg.total_threads = c["total_threads"] * c["workers"]
    cfg.plain_worker_kernel, cfg.relaxed_coherence, cfg.exact_reduction = c["plain_worker_kernel"], c["relaxed_coherence"], c["exact_reduction"]
    tn = None
    if c["tune"] is not None:
        tn = _lib.Tuning()
        tn.struct_size = C.sizeof(_lib.Tuning)
        tn.hot_rows_v = tn.hot_rows_u = tn.mem_mode = tn.atomic_rank = -1
        tn.hot_cap, tn.hot_weight_permille, tn.window_refresh = 128, 125, 16
        setattr(tn, *c["tune"])
    out = _lib.RowPlan()
    _lib.check(L.w2b_plan_rows(C.byref(cfg), C.byref(tn) if tn is not None else None, cn.ctypes.data_as(_lib.i64p),
                               c["num_cus"], c["workers"], C.byref(out)))
    return [getattr(out, k) for k in FIELDS]


def test_plan_grid_reproduces_the_recorded_decisions():
    L = _lib.lib()
    vocab = _vocabularies()
    cases = list(_cases())
    if os.environ.get("W2B_RECORD_PLAN_GRID") == "1":
        with open(PLAN_GRID_JSON, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(_plan(L, vocab, c), separators=(",", ":")) for c in cases) + "\n]\n")
    rec = json.load(open(PLAN_GRID_JSON))
    # the recording itself: large enough, and not a grid of zeros
    assert len(rec) == len(cases) >= 4000 and all(len(r) == len(FIELDS) == 9 for r in rec)
    assert os.path.getsize(PLAN_GRID_JSON) < 200_000
    col = {k: np.array([r[j] for r in rec]) for j, k in enumerate(FIELDS)}
    workers = np.array([c["workers"] for c in cases])
    share = {k: float(np.mean(col[k] != 0)) for k in FIELDS}
    share["concurrent_workers"] = float(np.mean(col["concurrent_workers"] < workers))
    print("plan grid: %d cases, %d distinct plans, share of cases with a non-trivial value: %s"
          % (len(rec), len({tuple(r) for r in rec}), {k: round(v, 3) for k, v in share.items()}))
    for k in ("copies_v", "atomic_rank_v", "atomic_rank_u", "full_device", "row_group_kernel"):
        assert share[k] >= 0.10, (k, share[k])
    for k in ("refresh_rows_u", "concurrent_workers"):
        assert share[k] >= 0.05, (k, share[k])
    # the library under test against it
    for i, (c, want) in enumerate(zip(cases, rec)):
        got = _plan(L, vocab, c)
        assert got == want, "case %d %r: %s, recorded %s" % (i, c, dict(zip(FIELDS, got)), dict(zip(FIELDS, want)))
