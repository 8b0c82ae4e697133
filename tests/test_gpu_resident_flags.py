"""-m gpu: the SENTENCE-RESIDENT worker kernel (word2bits_amd/csrc/w2b_kernels_resident.hip, `-window-cache 1`) under the flags
that tests/test_gpu_worker.py leaves out: -reg != 0, the run-time generic quantizer (bitlevel >= 3), the atomic target-row
form, and compute_loss off.  Of k_train_resident<QM, LOSS, MM, UC> that puts every value of each parameter under a bit
comparison (QM 0-3, LOSS on / off, MM 0 / 16 here and 8 through tests/test_gpu_bigtable.py, UC off / on), each with and
without -reg -- not every product of them: MM 16 runs with QM 0, 1, 2 and 3 and with LOSS off once, MM 8 with QM 1 and 3.

What these comparisons cannot see is arithmetic both kernels share (quant<3> and the other device functions of
w2b_device.hpp): a wrong level moves both sides alike.  That is what the oracle cases of test_gpu_worker.py are for.

The scheme is the one of test_sentence_resident_kernel_equals_plain_kernel_single_worker: one worker, 300 words, 6000 Zipf
tokens in sentences of 23 and one of 1100, three runs (resident at 333 positions per launch, plain at 333, resident at 50)
that must leave the same BITS in u and v, the same word count and alpha.  The plain kernel in turn meets the oracle with the
same flags in test_gpu_worker.py (test_single_worker_short_horizon_tight_reg_and_generic_quantizer).

With -reg the update of a context row is x + (err - 2 alpha reg x): a word that occurs twice in a window is updated twice
and the second update has to see the first (ref src/word2bits.cpp:494-503).  Its row lives in an LDS slot, in a register, or
(radius = window - 1) in both -- w2b_testlib.walk restates the reference's sentence reader and window draw on the host and the
tests assert that the stream really has such windows."""
import ctypes as C

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import row_sumsq_floor, walk, zipf_ids
from test_gpu_worker import token_stream, counts_of

pytestmark = pytest.mark.gpu

V, N, TABLE = 300, 6000, 50000
LOSS_REL = 1e-6          # "same terms, other order of addition" (test_gpu_groups.py test_row_group_kernel_with_regularisation)
_cache = {}


def stream():
    if "stream" not in _cache:
        rng = np.random.default_rng(9)
        ids = token_stream(rng, V, N, line=23)           # short sentences: many window fills / flushes
        ids[3000:4100] = zipf_ids(rng, V, 1100)          # and one sentence longer than 1000 tokens
        _cache["stream"] = (ids, counts_of(ids, V))
    return _cache["stream"]


def stream_walk(window, negative, sample=1e-3):
    key = ("walk", window, negative, sample)
    if key not in _cache:
        ids, cn = stream()
        _cache[key] = walk(ids, cn, window, negative, sample, TABLE)
    return _cache[key]


def plan_atomic_rank_v(t, cn):
    """atomic_rank_v of the launch plan of trainer `t`.  Not read back from the launch: re-planned from the trainer's own
    configuration, tuning and counts through w2b_plan_rows, the report tests/test_host_logic.py reads.  For window_cache=True
    that report plans as the plain kernel would, but the rank of v is decided before the kernel is (w2b_plan_launch, step 1),
    so it holds for the sentence-resident launch as well.  The number of CUs passed here (256) plays no part: an explicit
    atomic_rank is taken as it stands, and without one a single worker's rank is 0 whatever the device."""
    tn = _lib.Tuning()
    _lib.check(_lib.lib().w2b_get_tuning(t._h, C.byref(tn)))
    out = _lib.RowPlan()
    cn = np.ascontiguousarray(cn, np.int64)
    _lib.check(_lib.lib().w2b_plan_rows(C.byref(t.cfg), C.byref(tn), cn.ctypes.data_as(_lib.i64p), 256, t.num_threads, C.byref(out)))
    return out.atomic_rank_v


def run(D, window, negative, bitlevel, wc, pos, reg=0.0, loss=True, **tune):
    """one epoch of one worker on the shared stream; memoised (the plain run of a shape serves every test that needs it)"""
    key = ("run", D, window, negative, bitlevel, wc, pos, reg, loss, tuple(sorted(tune.items())),
           tuple(sorted(w2b.Trainer.default_tuning.items())))
    if key in _cache:
        return _cache[key]
    ids, cn = stream()
    t = w2b.Trainer(V, D, window, negative, bitlevel, num_threads=1, iter=1, sample=1e-3, reg=reg, train_words=int(cn.sum()),
                    compute_loss=loss, window_cache=wc, **tune)
    t.init_net()
    u0, v0 = t.get_model()
    t.set_vocab_counts(cn, TABLE)
    t.set_corpus(ids)
    t.set_shards(np.zeros(1, np.int64))
    r = dict(name=t.worker_kernel_name(), info=t.worker_kernel_info(), atomic_rank_v=plan_atomic_rank_v(t, cn), u0=u0, v0=v0)
    r["loss"] = t.train_epoch(positions_per_launch=pos)
    fin, r["wca"], r["alpha"], _ = t.epoch_status()
    assert fin
    r["u"], r["v"] = t.get_model()
    t.close()
    _cache[key] = r
    return r


def same_bits(a, b):
    return (a["wca"] == b["wca"] and a["alpha"] == b["alpha"]
            and np.array_equal(a["u"].view(np.uint32), b["u"].view(np.uint32))
            and np.array_equal(a["v"].view(np.uint32), b["v"].view(np.uint32)))


def three_runs(D, window, negative, bitlevel, reg=0.0, loss=True, **tune):
    """resident at 333 positions per launch, plain at 333, resident at 50"""
    res = [run(D, window, negative, bitlevel, wc, pos, reg, loss, **tune) for wc, pos in ((True, 333), (False, 333), (True, 50))]
    assert [r["name"] for r in res] == ["resident", "plain", "resident"]
    resident, radius, colb, _, _ = res[0]["info"]
    assert resident and colb == 16 and radius == (window - 1 if (D, window) == (768, 12) else window)
    return res


def regularisation_share(plain, D, window, negative, bitlevel, reg):
    """lower bound of the regularisation terms' share of the plain run's epoch loss: reg * sum q^2 for every row a centre
    word visits (ref :437-445, :463-471), the visits counted on the host, the row term bounded by the smallest one among the
    rows of the model before and after the epoch (bitlevel 1: q^2 = 1/9 whatever the row holds, so the bound is the term)"""
    trained, dups, rows_u, rows_v = stream_walk(window, negative)
    floor = row_sumsq_floor(bitlevel, plain["u0"], plain["v0"], plain["u"], plain["v"])
    if bitlevel == 1:
        assert floor == pytest.approx(D / 9.0, rel=1e-6)
    term = reg * floor * (rows_u + rows_v)
    return term / abs(plain["loss"]), dups, trained


# ------------------------------------------------------------------------------------------ 1. -reg != 0
REG_CASES = [
    (200, 8, 24, 1, 0), (200, 8, 24, 1, 8),
    (400, 8, 24, 2, 0),
    (64, 2, 3, 0, 0),
    (768, 12, 5, 1, 0), (768, 12, 5, 1, 8),      # radius window - 1: the outermost context rows are register-held
    (4, 3, 3, 2, 0),                             # one 16-byte column, the narrowest row the kernel accepts
    (260, 5, 5, 1, 0),                           # 65 columns: the second data wavefront holds one live lane
]


def hot_tune(hot):
    return dict(hot_rows_v=hot, hot_rows_u=hot, hot_period=2)


@pytest.mark.parametrize("D,window,negative,bitlevel,hot", REG_CASES)
def test_resident_equals_plain_with_regularisation(gpu, D, window, negative, bitlevel, hot):
    """-reg 1e-3, compute_loss on: the ar2 terms of the target-row update, the four forms of phase C (no slot twice / a slot
    twice or the register-held form / the two register-held outer rows) and the loss_reg bookkeeping.  Bits of u and v, word
    count and alpha equal; the epoch loss equal up to the order in which the regularisation terms are added -- and those
    terms are at least 100 x that tolerance of the loss, so a lost or doubled term cannot hide in it."""
    reg = 1e-3
    res = three_runs(D, window, negative, bitlevel, reg=reg, **hot_tune(hot))
    assert res[0]["info"][4] == (8 if hot == 8 else 0)
    share, dups, trained = regularisation_share(res[1], D, window, negative, bitlevel, reg)
    print("RESIDENT reg D=%d w=%d k=%d b=%d hot=%d: %d positions, %d with a repeated context word, reg share of the loss >= %.3g"
          % (D, window, negative, bitlevel, hot, trained, dups, share))
    assert dups >= 10                                   # the order-dependent case of phase C is really in the stream
    assert share >= 100 * LOSS_REL
    for k in (1, 2):
        assert same_bits(res[0], res[k])
        assert res[0]["loss"] == pytest.approx(res[k]["loss"], rel=LOSS_REL)
    assert not np.array_equal(res[0]["u"], res[0]["u0"]) and not np.array_equal(res[0]["v"], res[0]["v0"])


# ------------------------------------------------------------------------------------------ 2. generic quantizer
@pytest.mark.parametrize("D,window,negative,bitlevel,reg", [
    (64, 2, 3, 4, 0.0), (200, 8, 24, 8, 0.0),
    (96, 1, 2, 3, 0.0),          # bitlevel 3: every level is +-0
    (200, 8, 24, 4, 1e-3),
])
def test_resident_equals_plain_generic_quantizer(gpu, D, window, negative, bitlevel, reg):
    """bitlevel >= 3 is quant<3>, the run-time quantizer (QM == 3).  At bitlevel 3 every quantized value is +-0: the window
    average, every dot product and the error are zero, so without -reg no row may move at all."""
    res = three_runs(D, window, negative, bitlevel, reg=reg)
    for k in (1, 2):
        assert same_bits(res[0], res[k])
        assert res[0]["loss"] == pytest.approx(res[k]["loss"], rel=LOSS_REL)
    if reg:
        share, dups, _ = regularisation_share(res[1], D, window, negative, bitlevel, reg)
        print("RESIDENT generic+reg: reg share of the loss >= %.3g, %d windows with a repeated word" % (share, dups))
        assert dups >= 10 and share >= 100 * LOSS_REL
    for r in res:
        if bitlevel == 3:
            assert np.array_equal(r["u"], r["u0"]) and np.array_equal(r["v"], r["v0"])
        else:
            assert not np.array_equal(r["u"], r["u0"]) and not np.array_equal(r["v"], r["v0"])


# ------------------------------------------------------------------------------------------ 3. atomic target rows
@pytest.mark.parametrize("D,window,negative,bitlevel,reg,loss", [
    (800, 8, 24, 1, 0.0, True), (200, 8, 24, 2, 1e-3, True), (64, 2, 3, 0, 0.0, True),
    (64, 2, 3, 4, 0.0, True),            # k_train_resident<3, *, 16, false>: atomic rows under the run-time quantizer
    (200, 8, 24, 2, 1e-3, False),        # k_train_resident<*, false, 16, false>: atomic rows with the loss off
])
def test_resident_atomic_target_rows_equal_plain_stores(gpu, D, window, negative, bitlevel, reg, loss):
    """atomic_rank = V - 1: every target row's delta is added atomically (MM bit 4).  One worker has nobody to race with, an
    atomic add of d lands as fl(x + d): the bits of the sentence-resident kernel without the rank and of the plain kernel.
    That the MM = 16 instantiation is what ran is shown by what the launcher branches on: the kernel is the sentence-resident
    one, its radius is the window, the table is far below 2 GiB and the planned rank is positive."""
    atom = run(D, window, negative, bitlevel, True, 333, reg, loss, atomic_rank=V - 1)
    base = run(D, window, negative, bitlevel, True, 333, reg, loss)
    plain = run(D, window, negative, bitlevel, False, 333, reg, loss)
    assert (atom["name"], base["name"], plain["name"]) == ("resident", "resident", "plain")
    assert atom["info"][1] == window                      # the atomic form exists for radius == window only
    assert atom["atomic_rank_v"] == V - 1 and base["atomic_rank_v"] == 0 and plain["atomic_rank_v"] == 0
    assert same_bits(atom, base) and same_bits(atom, plain)
    if loss:
        assert atom["loss"] == pytest.approx(base["loss"], rel=LOSS_REL) and atom["loss"] == pytest.approx(plain["loss"], rel=LOSS_REL)
    else:
        assert same_bits(atom, run(D, window, negative, bitlevel, True, 333, reg, True, atomic_rank=V - 1))
    assert not np.array_equal(atom["v"], atom["v0"])


def test_resident_with_atomic_rows_and_short_radius_runs_the_plain_kernel(gpu):
    """radius window - 1 has no atomic form (w2b_resident_atomic_ok): the launch plan takes the plain kernel, which adds at run time"""
    ids, cn = stream()
    for kw, want in ((dict(), "resident"), (dict(atomic_rank=V - 1), "plain")):
        t = w2b.Trainer(V, 768, 12, 5, 1, num_threads=1, iter=1, train_words=int(cn.sum()), window_cache=True, **kw)
        t.set_vocab_counts(cn, TABLE)
        assert t.worker_kernel_name() == want, kw
        assert plan_atomic_rank_v(t, cn) == (V - 1 if kw else 0)
        assert t.worker_kernel_info()[1] == (11 if want == "resident" else -1)
        t.close()


# ------------------------------------------------------------------------------------------ 4. LOSS = false
@pytest.mark.parametrize("D,window,negative,bitlevel", [(200, 8, 24, 1), (768, 12, 5, 1)])
def test_resident_values_do_not_depend_on_compute_loss(gpu, D, window, negative, bitlevel):
    """compute_loss off selects the LOSS = false instantiations (no regsq, no loss_reg): same bits as with it on"""
    on = run(D, window, negative, bitlevel, True, 333, 1e-3, True, **hot_tune(0))
    off = run(D, window, negative, bitlevel, True, 333, 1e-3, False, **hot_tune(0))
    plain_off = run(D, window, negative, bitlevel, False, 333, 1e-3, False, **hot_tune(0))
    assert (on["name"], off["name"], plain_off["name"]) == ("resident", "resident", "plain")
    assert same_bits(on, off) and same_bits(off, plain_off)
    assert on["loss"] < 0.0
