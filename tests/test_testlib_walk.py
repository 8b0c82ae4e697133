"""w2b_testlib.walk (the host restatement of what one reference worker visits, which the -reg tests of test_gpu_worker.py,
test_gpu_resident_flags.py and test_gpu_groups_flags.py use to show that the regularisation terms are large against their loss
tolerance) against the oracle itself, on the two token streams and at every (window, negative, sample) those tests walk -- and
what test_gpu_groups_flags.py assumes of its inputs: windows that hold a word twice, hot rows that are a real share of the stream.

The oracle reports no counts, but with -alpha 0 no row moves, so its epoch loss is a linear function of them with
coefficients known on the host.  Rows of four equal values, bitlevel 0 (the quantizer is the identity):
  u = 1/2, v = 0,   reg 1:  every context row books -1, every target row log sigmoid(0)          -> context rows visited
  u = 0,   v = 1/2, reg 1:  every target row books log sigmoid(0) - 1                             -> target rows visited
  u = 1/2, v = 1/2, reg 0:  the centre word books log sigmoid(1), a negative one log sigmoid(-1)  -> positions trained"""
import numpy as np
import pytest

from w2b_testlib import OracleState, walk
import test_gpu_groups_flags
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
    ("flags", 8, 12, 1e-3), ("flags", 16, 8, 1e-3),       # test_gpu_groups_flags.py REG_CASES
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


def test_row_group_reg_cases_have_windows_with_a_repeated_word():
    """every (window, negative) of test_gpu_groups_flags.REG_CASES: the loop of phase C that feeds an updated row back into its
    next delta only runs for a word that occurs more than once in a window.  With every row a lossless add all of those go
    through add_cols_group; with atomic_rank_u = 25 both forms must meet one: a repeated word among rows 1 .. 25 (added) and
    one above (stored)."""
    ids, cn = test_gpu_resident_flags.stream()
    shapes = sorted({(w, k) for _, w, k, _, _ in test_gpu_groups_flags.REG_CASES})
    assert shapes == [(2, 3), (8, 12), (8, 24), (16, 8)]
    for window, negative in shapes:
        words = {}
        trained, dups, rows_u, rows_v = walk(ids, cn, window, negative, 1e-3, test_gpu_resident_flags.TABLE, dup_words=words)
        assert (trained, dups, rows_u, rows_v) == test_gpu_resident_flags.stream_walk(window, negative)
        print("walk w=%d k=%d: %d positions, %d with a repeated context word (%d distinct words)" % (window, negative, trained, dups, len(words)))
        assert dups > 0 and words and dups <= sum(words.values()) and max(words.values()) <= dups
        assert all(1 <= w < test_gpu_resident_flags.V for w in words)
        if (window, negative) == (8, 24):
            ranks = {kn["atomic_rank_u"] for *_, kn in test_gpu_groups_flags.REG_CASES if 0 < kn.get("atomic_rank_u", 0) < 299}
            assert ranks == {25}
            assert sum(n for w, n in words.items() if w <= 25) > 0 and sum(n for w, n in words.items() if w > 25) > 0


def test_refreshed_rows_are_a_real_share_of_the_stream():
    """test_gpu_groups_flags.COPY_CASES: rows 1 .. refresh_rows_u are at least 10 % of the tokens (Zipf over 299 words: word 1
    alone is 1 / H_299 = 16 % of the draws and, sentence ends counted, 15 % of the tokens), so a wrong copy is read at one position in ten at the least, and as a context
    row in most windows"""
    ids, _ = test_gpu_resident_flags.stream()
    shares = {r: test_gpu_groups_flags.hot_share(r) for r in sorted({c[4] for c in test_gpu_groups_flags.COPY_CASES})}
    print("share of the stream's tokens among rows 1 .. n:", shares)
    assert sorted(shares) == [1, 3, 4, 5, 64]
    assert all(s >= 0.10 for s in shares.values())
    assert shares[1] == np.count_nonzero(ids == 1) / len(ids) and shares[64] > shares[5] > shares[4] > shares[3] > shares[1]
