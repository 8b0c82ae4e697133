"""-m gpu: the lean worker kernel's row predicates, where tests/test_gpu_worker_lean.py does not look.

In the lean form of process_word (w2b_device.hpp) the lane predicate is an offset: a lane beyond the row passes an offset that
is out of range for every buffer resource of the kernel, and the hardware bounds check drops its access.  The stores of phase
C's stash slots take their row predicate (inside the window, first occurrence, not read again) in the same way; phase C itself
runs in two passes, stash slots first, then the rows that are read again.  If a predicate were wrong, nothing would fault --
every access is made with the id of a real row -- but bits would differ: a store that is not dropped lands in the first
columns of the NEXT row or writes a row that must not change, and a load that is not dropped brings another row's values into
the arithmetic.

Same harness as the lean / generic file: one worker, V = 40, 300 positions from InitNet and then the rest of the epoch, the lean
form against a trainer created under W2B_GENERIC_WORKER=1, all of u and v (and loss, words, alpha) bit for bit.  On top, every
case here plants canary rows before training (plant_canaries): the rows that no list can name must hold their pattern to the
bit afterwards.

Which rows those are, from the token stream and the draw rules:
  * row 0 is "</s>": the sentence reader ends a sentence there and never hands it out, so it is neither a centre word nor a
    context word, and a negative draw that hits 0 is redrawn from 1 .. V - 1 (ref src/word2bits.cpp:456-458).  Rows 0 of u and
    of v are never read or written.
  * word V - 1 is not in the stream: never a context word, so row V - 1 of u is untouched; never a centre word either, but the
    unigram table and the redraw above both reach it, so row V - 1 of v IS a negative target and is only compared.
[u | v] is one allocation: the row after row V - 1 of u is row 0 of v, and rows V - 2 of u / V - 2 of v, which the stream does
train, sit right before a canary.  At D = 8 one wavefront has two live lanes and 62 idle ones, whose stores would cover the next
31 rows; at D = 260 the second wavefront has one live lane; at D = 800 the last 56 lanes of 256 are idle.
"""
import numpy as np
import pytest

from test_gpu_worker_lean import V, both

pytestmark = pytest.mark.gpu

CANARY = 0x3C5A0000       # + 4096 * (2 * table + (row != 0)) + column: floats near 0.0133, tame as targets of a dot product


def canary(tab, row, D):
    return (CANARY + 4096 * (2 * tab + (1 if row else 0)) + np.arange(D)).astype(np.uint32)


def plant_canaries(t):
    """a recognisable bit pattern into rows 0 and V - 1 of u and of v, through the device view of the tables"""
    import torch
    m = t.model_tensor().view(2, V, -1)
    D = m.shape[2]
    for tab in (0, 1):
        for row in (0, V - 1):
            m[tab, row, :] = torch.from_numpy(canary(tab, row, D).view(np.float32)).to(m.device)
    torch.cuda.synchronize()
    got = m.cpu().numpy().view(np.uint32)
    assert (got[1, V - 1] == canary(1, V - 1, D)).all()


def check(monkeypatch, D, window, negative, bitlevel, loss=True, **tuning):
    r = both(monkeypatch, D, window, negative, bitlevel, loss, poke=plant_canaries, **tuning)     # (lean == generic, and lean ran)
    for k in ("u", "u2"):
        tab = r[k].reshape(V, D)
        assert (tab[0] == canary(0, 0, D)).all(), (k, 0)
        assert (tab[V - 1] == canary(0, V - 1, D)).all(), (k, V - 1)
    for k in ("v", "v2"):
        tab = r[k].reshape(V, D)
        assert (tab[0] == canary(1, 0, D)).all(), (k, 0)
    return r


# per-XCD copies of rows 1..4 of both tables, merged every second centre word: the hot / master branch of every access, with
# short chunks (negative 5), cut chunks (V = 40: targets repeat) and partly filled wavefronts
@pytest.mark.parametrize("bitlevel", [0, 1, 2])
@pytest.mark.parametrize("negative", [5, 24])
@pytest.mark.parametrize("D", [8, 260, 800])
def test_hot_copies_short_chunks_partial_wavefronts(gpu, monkeypatch, D, negative, bitlevel):
    r = check(monkeypatch, D, 8, negative, bitlevel, hot_rows_u=4, hot_rows_v=4, hot_period=2)
    assert r["hot"] == 4


# phase C reads a context row again instead of taking it from the LDS stash: rows 1..fresh_rank_u, and every context row
# beyond the first W2B_STASH = 8 of a window (window 8: up to 16)
@pytest.mark.parametrize("tuning", [dict(fresh_rank_u=10), dict()], ids=["fresh_rank_u", "beyond_stash"])
@pytest.mark.parametrize("D", [260, 800])
def test_phase_c_rereads(gpu, monkeypatch, D, tuning):
    check(monkeypatch, D, 8, 5, 1, **tuning)


# one negative, window 1: chunks of at most 2 rows (11 slots of 13 beyond the chunk), at most 2 context rows of 8 slots, and
# often a single one
@pytest.mark.parametrize("bitlevel", [0, 1, 2])
@pytest.mark.parametrize("D", [8, 260, 800])
def test_nearly_empty_chunks(gpu, monkeypatch, D, bitlevel):
    check(monkeypatch, D, 1, 1, bitlevel)
