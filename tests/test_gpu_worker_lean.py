"""-m gpu: the lean form of the plain worker kernel (process_word<..., LEAN>, w2b_device.hpp) against its generic form.

The lean form runs 16-byte columns, coherent rows, tables below 2 GiB, no atomic rows, reg == 0 and bitlevel 0..2; it leaves
out the regularisation terms, the atomic-add paths and, at one bit, the products with the quantized value.  None of that may
change a bit: every case runs one worker for 300 positions from InitNet twice, once in the lean form and once in a trainer
created under W2B_GENERIC_WORKER=1 (the variable is read when a trainer is created), and compares ALL of u, ALL of v, the loss
sum, the words done and alpha bit for bit -- after the 300 positions, and again at the end of the epoch.

V = 40: targets repeat inside a centre word (chunks are cut), negative draws hit the centre word (skipped), context rows repeat
inside a window (one update per occurrence).  A sentence end every 50 tokens cuts the windows.
"""
import numpy as np
import pytest

import word2bits_amd as w2b

pytestmark = pytest.mark.gpu

V, POSITIONS, LINE = 40, 300, 50


def token_stream():
    rng = np.random.default_rng(11)
    n = 440                                    # eight whole sentences: 300 positions end inside the epoch, a second launch finishes it
    ids = rng.integers(1, V - 1, n).astype(np.int32)    # (word V - 1 is never in the stream: its row of v is a negative target only)
    ids[LINE - 1::LINE] = 0                    # "</s>"
    return ids


IDS = token_stream()
CN = np.maximum(np.bincount(IDS, minlength=V), 1).astype(np.int64)
CN[1:] = np.sort(CN[1:])[::-1]                 # (the vocabulary is sorted by count; the ids are just labels here)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(monkeypatch, generic, D, window, negative, bitlevel, loss, reg=0.0, poke=None, **tuning):
    """one worker, InitNet, 300 positions, then the rest of the epoch; returns what the two forms must agree on"""
    # (automatic atomic rows would take every row of a 40-word vocabulary, and with them the generic form: none, unless a case asks)
    tuning = dict(dict(atomic_rank=0), **tuning)
    if generic:
        monkeypatch.setenv("W2B_GENERIC_WORKER", "1")
    else:
        monkeypatch.delenv("W2B_GENERIC_WORKER", raising=False)
    t = w2b.Trainer(V, D, window, negative, bitlevel, num_threads=1, iter=1, sample=0.0, reg=reg, train_words=int(CN.sum()),
                    compute_loss=loss, window_cache=False, **tuning)
    try:
        t.init_net()
        if poke is not None:
            poke(t)
        t.set_vocab_counts(CN, 5000)
        t.set_corpus(IDS)
        t.set_shards(np.zeros(1, np.int64))
        assert t.worker_kernel_name() == "plain"
        lean = t.worker_kernel_lean()
        t.epoch_begin()
        t.train_step(POSITIONS)
        u, v = t.get_model()
        fin, wca, alpha, lsum = t.epoch_status()
        assert not fin
        t.train_step(POSITIONS)
        u2, v2 = t.get_model()
        fin2, wca2, alpha2, lsum2 = t.epoch_status()
        assert fin2
        hot = t.worker_kernel_info()[4]
    finally:
        t.close()
    return dict(lean=lean, hot=hot, u=bits(u), v=bits(v), state=(wca, bits(np.float32(alpha)).item(), np.float64(lsum).view(np.uint64).item()),
                u2=bits(u2), v2=bits(v2), state2=(wca2, bits(np.float32(alpha2)).item(), np.float64(lsum2).view(np.uint64).item()))


def both(monkeypatch, D, window, negative, bitlevel, loss, expect_lean=True, **kw):
    lean = run(monkeypatch, False, D, window, negative, bitlevel, loss, **kw)
    gen = run(monkeypatch, True, D, window, negative, bitlevel, loss, **kw)
    assert lean["lean"] == expect_lean and not gen["lean"]
    for k in ("u", "v", "u2", "v2"):
        bad = np.argwhere(lean[k] != gen[k])
        assert bad.size == 0, (k, len(bad), bad[:4].tolist())
    assert lean["state"] == gen["state"] and lean["state2"] == gen["state2"]
    if loss:
        assert lean["state2"][2] != 0                      # (a loss was booked at all)
    assert lean["u2"].tobytes() != lean["u"].tobytes()     # (and the second launch trained)
    return lean


# dim 8: one partly filled lane group; 200: one wavefront, 50 lanes; 260: 65 columns, the wavefront edge; 800: the headline row
# window 8: more than W2B_CA = 8 context rows; negative 5: one short chunk; negative 24: 13 + 12
@pytest.mark.parametrize("loss", [True, False])
@pytest.mark.parametrize("bitlevel", [0, 1, 2])
@pytest.mark.parametrize("negative", [5, 24])
@pytest.mark.parametrize("window", [2, 8])
@pytest.mark.parametrize("D", [8, 200, 260, 800])
def test_lean_equals_generic(gpu, monkeypatch, D, window, negative, bitlevel, loss):
    both(monkeypatch, D, window, negative, bitlevel, loss)


ZERO_COLS = (1, -2)       # columns that poke_zeros clears in every row


def poke_zeros(t):
    """+0.0, -0.0 and negative elements into rows of u and v, through the device view of the tables; and two columns that
    are zero in EVERY row: +0.0 / -0.0 by turns in u, -0.0 in v"""
    m = t.model_tensor().view(2, V, -1)
    import torch
    D = m.shape[2]
    pat = torch.tensor([0.0, -0.0, -0.25, -1e-3, 0.5, -0.0], dtype=torch.float32, device=m.device)
    for tab in (0, 1):
        for row in range(1, V, 2):
            reps = (D + len(pat) - 1) // len(pat)
            m[tab, row, :] = pat.roll(row + tab).repeat(reps)[:D]
    for c in ZERO_COLS:
        m[0, 0::2, c] = 0.0
        m[0, 1::2, c] = -0.0
        m[1, :, c] = -0.0
    torch.cuda.synchronize()
    got = bits(m.cpu().numpy())
    assert (got == 0x80000000).any() and (got == 0).any()


@pytest.mark.parametrize("bitlevel", [0, 1, 2])
@pytest.mark.parametrize("D,window,negative", [(200, 8, 24), (8, 2, 5)])
def test_lean_equals_generic_signed_zeros(gpu, monkeypatch, D, window, negative, bitlevel):
    """rows that hold +0.0, -0.0 and negative values: where `x - 0 * x` and `x` could differ (w2b_device.hpp, LEAN) -- a -0.0
    element of a v row that receives a -0.0 update (an element of the window average that is +0, times g < 0).

    At bitlevel 0 the cleared columns make that case certain and keep it visible: the window average is +0 there for every
    centre word, so every negative target gets the delta -0 and every centre word +0, and the columns stay zero in both tables.
    Row V - 1 of v is only ever a negative target: its -0.0 elements become +0.0 through `x + (-0 - 0 * x)`, the one place where
    leaving the regularisation term out would show (x + -0 stays -0.0)."""
    r = both(monkeypatch, D, window, negative, bitlevel, True, poke=poke_zeros)
    if bitlevel == 0:
        v2 = r["v2"].reshape(V, D)
        for c in ZERO_COLS:
            assert (v2[:, c] & 0x7fffffff == 0).all()
            assert v2[V - 1, c] == 0, hex(int(v2[V - 1, c]))     # (was 0x80000000: the row was drawn, and the delta was -0)


@pytest.mark.parametrize("bitlevel", [0, 1, 2])
def test_lean_equals_generic_with_hot_row_copies(gpu, monkeypatch, bitlevel):
    """the per-XCD copies of the hottest rows are read and written by the lean form as by the generic one"""
    r = both(monkeypatch, 200, 8, 24, bitlevel, True, hot_rows_v=4, hot_rows_u=4, hot_period=2)
    assert r["hot"] == 4


@pytest.mark.parametrize("reg,bitlevel", [(1e-3, 1), (1e-3, 0), (0.0, 4)])
def test_generic_form_runs_outside_the_lean_shape(gpu, monkeypatch, reg, bitlevel):
    """-reg != 0 and the run-time quantizer are the generic form's: the library says so, and the switch changes nothing"""
    both(monkeypatch, 200, 8, 24, bitlevel, True, reg=reg, expect_lean=False)


@pytest.mark.parametrize("tuning", [dict(atomic_rank=10), dict(atomic_rank=0, atomic_rank_u=10), dict(force_row_desc=1)])
def test_generic_form_runs_with_atomic_rows_and_row_descriptors(gpu, monkeypatch, tuning):
    both(monkeypatch, 200, 8, 24, 1, True, expect_lean=False, **tuning)


def test_generic_form_runs_with_relaxed_rows(gpu, monkeypatch):
    monkeypatch.delenv("W2B_GENERIC_WORKER", raising=False)
    t = w2b.Trainer(V, 200, 8, 24, 1, num_threads=1, iter=1, sample=0.0, train_words=int(CN.sum()), window_cache=False,
                    relaxed_coherence=True, atomic_rank=0)
    try:
        t.set_vocab_counts(CN, 5000)
        assert t.worker_kernel_name() == "plain" and not t.worker_kernel_lean()
    finally:
        t.close()
