"""w2b_testlib.walk (the host restatement of what one reference worker visits, which the -reg tests of test_gpu_worker.py and
test_gpu_resident_flags.py use to show that the regularisation terms are large against their loss tolerance) against the
oracle itself, on the two token streams and at every (window, negative, sample) those tests walk.

The oracle reports no counts, but with -alpha 0 no row moves, so its epoch loss is a linear function of them with
coefficients known on the host.  Rows of four equal values, bitlevel 0 (the quantizer is the identity):
  u = 1/2, v = 0,   reg 1:  every context row books -1, every target row log sigmoid(0)          -> context rows visited
  u = 0,   v = 1/2, reg 1:  every target row books log sigmoid(0) - 1                             -> target rows visited
  u = 1/2, v = 1/2, reg 0:  the centre word books log sigmoid(1), a negative one log sigmoid(-1)  -> positions trained"""
import numpy as np
import pytest

from w2b_testlib import OracleState, walk
import test_gpu_resident_flags
import test_gpu_worker


def worker_stream():
    """the stream of test_gpu_worker.short_horizon_tight"""
    ids = test_gpu_worker.token_stream(np.random.default_rng(4), 5000, 3000)
    return ids, test_gpu_worker.counts_of(ids, 5000)


def oracle_loss(ids, cn, window, negative, sample, uval, vval, reg):
    D = 4
    o = OracleState(cn, D, window=window, negative=negative, bitlevel=0, num_threads=1, iters=1, alpha=0.0, sample=sample,
                    reg=reg, table_size=50000, init=False)
    o.m.train_words = int(cn.sum())
    o.u[:] = uval
    o.v[:] = vval
    loss = o.train_epoch_tokens(ids, np.zeros(1, np.int64))
    assert (o.u == np.float32(uval)).all() and (o.v == np.float32(vval)).all()       # -alpha 0: nothing moved
    return loss


@pytest.mark.parametrize("which,window,negative,sample", [
    ("flags", 8, 24, 1e-3), ("flags", 2, 3, 1e-3), ("flags", 12, 5, 1e-3), ("flags", 3, 3, 1e-3), ("flags", 5, 5, 1e-3),
    ("worker", 8, 24, 0.0), ("worker", 3, 7, 0.0), ("worker", 8, 24, 1e-3),
])
def test_walk_counts_what_the_oracle_visits(which, window, negative, sample):
    ids, cn = test_gpu_resident_flags.stream() if which == "flags" else worker_stream()
    trained, dups, rows_u, rows_v = walk(ids, cn, window, negative, sample, 50000)
    assert 0 < dups <= trained <= rows_v <= trained * (negative + 1) and trained <= rows_u <= trained * 2 * window
    ls = [float(np.log(np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-x))))) for x in (0.0, 1.0, -1.0)]
    # each sum has fewer than 2e5 terms of size <= 1.4, known to a float ulp: the counts come out to well under 1/2
    got_v = oracle_loss(ids, cn, window, negative, sample, 0.0, 0.5, 1.0) / (ls[0] - 1.0)
    got_u = -(oracle_loss(ids, cn, window, negative, sample, 0.5, 0.0, 1.0) - rows_v * ls[0])
    got_t = (oracle_loss(ids, cn, window, negative, sample, 0.5, 0.5, 0.0) - rows_v * ls[2]) / (ls[1] - ls[2])
    assert abs(got_v - rows_v) < 0.1 and abs(got_u - rows_u) < 0.1 and abs(got_t - trained) < 0.1, (got_v, got_u, got_t)
