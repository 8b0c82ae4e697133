"""-m gpu: the ROW-GROUP worker kernel (word2bits_amd/csrc/w2b_kernels_groups.hip, `row_groups=True`) under the flags and at the
shapes that tests/test_gpu_groups.py leaves out: compute_loss off, -reg != 0 beyond three cells (the generic quantizer, short
launches, every context row a lossless add, sub-sampling on), windows above 8 at two and four wavefronts per row (the second
trip of the context-row load), row lengths that leave a data wavefront nearly or wholly idle, and the refreshed read copies
of the hottest context rows (k_refresh_rows) to the exact epoch loss.

Of k_train_groups<QM, LOSS, RW, G, TC> -- (RW, G, TC) is (1, 4, 7), (2, 4, 7) or (4, 3, 9), chosen by the row length -- this
puts every value of each parameter under a bit comparison with the plain kernel: QM 0-3, LOSS on and off, RW 1, 2 and 4,
each with and without -reg.  Not every product of them:
  LOSS off runs as (QM, RW) = (1, 1), (2, 2), (0, 4), (3, 1), (1, 4), the first and the last with every row a lossless add
           too, and (2, 2) with -reg as well;
  -reg     runs as (1, 1), (2, 2), (0, 4), (1, 4), (2, 4), (3, 1) (bitlevel 4 and 8), with every row a lossless add as
           (1, 1), (0, 4), (3, 1);
  the run-time quantizer (QM 3) meets RW 1 only, here and in test_gpu_groups.py: <3, *, 2, 4, 7> and <3, *, 4, 3, 9> run in
           no test;
  the two-trip context-row load runs as (1, 2), (2, 4), (0, 4) -- RW 1 has it in test_gpu_groups.py at (256, 16, 27).

What these comparisons cannot see is arithmetic that both kernels share (quant<QM>, grad_scalar, log_sigmoid_term, wave_sum
and the other device functions of w2b_device.hpp): a wrong level moves both sides alike.  That is what the oracle cases are
for: test_gpu_worker.py pins the plain kernel, and test_gpu_groups.py the row-group kernel itself, to the CPU oracle -- with
-reg and bitlevel 4 / 8 in test_row_group_kernel_short_horizon_tight_reg_and_generic_quantizer.

The scheme is the one of test_gpu_resident_flags.py, whose stream, same_bits and LOSS_REL are used as they are: one worker,
300 words, 6000 Zipf tokens in sentences of 23 and one of 1100, sub-sampling 1e-3, three runs (row groups at 333 positions per
launch, plain at 333, row groups at 50: worker save / restore and the producer wavefront's one-word lead) that must leave the
same BITS in u and v, the same word count and alpha.  Without -reg the epoch loss is equal exactly (the log-sigmoid terms are
booked lane by lane as in the plain kernel); with -reg it is equal to LOSS_REL, the regularisation terms being summed per
group, and those terms are asserted to be at least 100 x LOSS_REL of the loss, so a lost or doubled term cannot hide in it.

With -reg the update of a context row is x + (err - 2 alpha reg x): a word that occurs m times in a window is updated m
times and every update has to see the one before (ref src/word2bits.cpp:494-503; the loop over k in phase C).  That the
stream has such windows at every (window, negative) used here, among the rows that get lossless adds and among those that
are stored, is asserted without a GPU in tests/test_testlib_walk.py.

Every shape below selects the row-group kernel as it stands: none needs more than the 160 KiB of LDS that w2b_groups_ok
admits, so no `negative` had to be lowered."""
import numpy as np
import pytest

import word2bits_amd as w2b
from test_gpu_resident_flags import V, TABLE, LOSS_REL, stream, same_bits, regularisation_share

pytestmark = pytest.mark.gpu

# no knobs ("auto"): the launch plan decides -- one worker stores every row of v and all but the few hottest rows of u, which get
# lossless adds from the adder wavefront (w2b_plan.cpp atomic_rows_u)
ALL_ATOMIC = dict(atomic_rank=V - 1, atomic_rank_u=V - 1)      # every row of v and of u gets lossless adds
_cache = {}


def ident(val):
    if isinstance(val, dict):
        return "-".join("%s%d" % (k.replace("atomic_rank", "ar"), v) for k, v in sorted(val.items())) or "auto"
    return None


def run(D, window, negative, bitlevel, groups, pos, reg=0.0, loss=True, **tune):
    """one epoch of one worker on the shared stream; memoised (a run serves every test that needs it)"""
    key = ("run", D, window, negative, bitlevel, groups, pos, reg, loss, tuple(sorted(tune.items())),
           tuple(sorted(w2b.Trainer.default_tuning.items())))
    if key in _cache:
        return _cache[key]
    ids, cn = stream()
    t = w2b.Trainer(V, D, window, negative, bitlevel, num_threads=1, iter=1, sample=1e-3, reg=reg, train_words=int(cn.sum()),
                    compute_loss=loss, row_groups=groups, **tune)
    t.init_net()
    r = dict(name=t.worker_kernel_name())
    r["u0"], r["v0"] = t.get_model()
    t.set_vocab_counts(cn, TABLE)
    t.set_corpus(ids)
    t.set_shards(np.zeros(1, np.int64))
    r["loss"] = t.train_epoch(positions_per_launch=pos)
    fin, r["wca"], r["alpha"], _ = t.epoch_status()
    assert fin
    r["u"], r["v"] = t.get_model()
    t.close()
    _cache[key] = r
    return r


def three_runs(D, window, negative, bitlevel, reg=0.0, loss=True, **tune):
    """row groups at 333 positions per launch, plain at 333, row groups at 50"""
    res = [run(D, window, negative, bitlevel, g, pos, reg, loss, **tune) for g, pos in ((True, 333), (False, 333), (True, 50))]
    assert [r["name"] for r in res] == ["groups", "plain", "groups"]
    return res


def moved(r):
    return not np.array_equal(r["u"], r["u0"]) and not np.array_equal(r["v"], r["v0"])


# ------------------------------------------------------------------------------------------ a. LOSS = false
LOSS_OFF_CASES = [
    (200, 8, 24, 1, 0.0, {}), (400, 8, 24, 2, 0.0, {}), (800, 8, 24, 0, 0.0, {}), (64, 2, 3, 4, 0.0, {}),
    (200, 8, 24, 1, 0.0, ALL_ATOMIC), (800, 8, 24, 1, 0.0, ALL_ATOMIC),
    (400, 8, 24, 2, 1e-3, {}),
]


@pytest.mark.parametrize("D,window,negative,bitlevel,reg,knobs", LOSS_OFF_CASES, ids=ident)
def test_row_groups_with_the_loss_off(gpu, D, window, negative, bitlevel, reg, knobs):
    """compute_loss off selects the k_train_groups<*, false, ...> instantiations (no fs, no regsq, no adder bookkeeping): the
    three runs agree bit for bit, and their rows are the rows of the same row-group run with the loss on -- u and v must not
    depend on LOSS."""
    res = three_runs(D, window, negative, bitlevel, reg=reg, loss=False, **knobs)
    for k in (1, 2):
        assert same_bits(res[0], res[k])
    on = run(D, window, negative, bitlevel, True, 333, reg, True, **knobs)
    assert on["name"] == "groups"
    assert same_bits(res[0], on)
    assert on["loss"] < 0.0
    assert moved(res[0])


# ------------------------------------------------------------------------------------------ b. shapes never run
WIDE_WINDOWS = [(512, 16, 24, 1), (800, 16, 8, 2), (1024, 12, 5, 0)]      # more context rows than a group loads in one trip
SHAPES = WIDE_WINDOWS + [
    (512, 8, 27, 2),        # negative + 1 = G * TC = 28: every register slot of the two-wavefront form is taken
    (4, 5, 5, 1),           # one 16-byte column: one live lane, the narrowest row w2b_groups_ok admits
    (252, 8, 24, 1),        # the last lane of the one wavefront idle
    (260, 8, 24, 2),        # 65 columns: the second wavefront of a row has one
    (516, 8, 12, 1),        # 129 columns: the third wavefront has one, the fourth none -- and takes part in every barrier,
                            # in add_cols_group and (EC = 2) in the error sum
    (1020, 3, 26, 0),       # the last lane of the fourth wavefront idle
]


@pytest.mark.parametrize("knobs", [dict(), ALL_ATOMIC], ids=ident)
@pytest.mark.parametrize("D,window,negative,bitlevel", SHAPES)
def test_row_groups_equal_plain_at_wide_windows_and_odd_row_lengths(gpu, D, window, negative, bitlevel, knobs):
    """no -reg, loss on: u, v, word count and alpha bit for bit and the epoch loss exactly, as
    test_gpu_groups.py test_row_group_kernel_equals_plain_kernel_single_worker has it.  Window 16 / 12 at RW = 2 / 4: up to
    32 / 24 context rows, of which a group stages 4 x 4 (G = 4) or 6 x 3 (G = 3) per trip, so the second trip of the load and
    the tail loops of the window average (LA) and of the error sum (LE) run.  With every row a lossless add the idle
    wavefronts and lanes pass zeros through add_cols_group, and the adder wavefront covers dim = 4 ... 1020."""
    res = three_runs(D, window, negative, bitlevel, **knobs)
    for k in (1, 2):
        assert same_bits(res[0], res[k])
        assert res[0]["loss"] == res[k]["loss"]
    assert res[0]["loss"] < 0.0 and moved(res[0])


# ------------------------------------------------------------------------------------------ c. -reg != 0
REG = 1e-3
REG_CASES = [
    (200, 8, 24, 1, {}), (400, 8, 24, 2, {}), (800, 8, 24, 0, {}), (516, 8, 12, 1, {}), (64, 2, 3, 4, {}), (200, 8, 24, 8, {}),
    (800, 16, 8, 2, {}),
    (200, 8, 24, 1, ALL_ATOMIC), (800, 8, 24, 0, ALL_ATOMIC), (64, 2, 3, 4, ALL_ATOMIC),      # phase C: by_add && reg_on only
    (200, 8, 24, 1, dict(atomic_rank_u=25, atomic_rank=0)),                                   # ... and both forms side by side
]


@pytest.mark.parametrize("D,window,negative,bitlevel,knobs", REG_CASES, ids=ident)
def test_row_groups_equal_plain_with_regularisation(gpu, D, window, negative, bitlevel, knobs):
    """-reg 1e-3, sub-sampling on, launches of 333 and of 50 positions: the ar2 terms of the target-row update (stored and
    added), phase C with the delta depending on the row -- fed back m times for a word that occurs m times in the window,
    by store and by add_cols_group --, the regsq bookkeeping of every group.  Bits of u and v, word count and alpha equal;
    the epoch loss equal up to the order in which the regularisation terms are added, and those terms are at least 100 x
    that tolerance of the loss."""
    res = three_runs(D, window, negative, bitlevel, reg=REG, **knobs)
    share, dups, trained = regularisation_share(res[1], D, window, negative, bitlevel, REG)
    print("GROUPS reg D=%d w=%d k=%d b=%d %s: %d positions, %d with a repeated context word, reg share of the loss >= %.3g; "
          "loss %.9g / %.9g / %.9g" % (D, window, negative, bitlevel, ident(knobs), trained, dups, share,
                                       res[0]["loss"], res[1]["loss"], res[2]["loss"]))
    assert dups > 0                                     # the order-dependent case of phase C is really in the stream
    assert share >= 100 * LOSS_REL
    for k in (1, 2):
        assert same_bits(res[0], res[k])
        assert res[0]["loss"] == pytest.approx(res[k]["loss"], rel=LOSS_REL)
    assert moved(res[0])


# ------------------------------------------------------------------------------------------ d. read copies, exactly
COPY_CASES = [(200, 8, 24, 1, 1), (200, 8, 24, 1, 3), (200, 8, 24, 1, 5), (200, 8, 24, 1, 64), (800, 8, 24, 2, 4), (36, 5, 5, 0, 4)]
COPY_POSITIONS = 2000


def hot_share(rows):
    """share of the shared stream's tokens that are words 1 .. rows (no sub-sampling: every token is a position)"""
    ids, _ = stream()
    return float(np.count_nonzero((ids >= 1) & (ids <= rows))) / len(ids)


def frozen_run(D, window, negative, bitlevel, refresh):
    """one epoch with alpha = 0 on a seeded random model: nothing moves, the loss is a function of the rows read"""
    key = ("frozen", D, window, negative, bitlevel, refresh)
    if key in _cache:
        return _cache[key]
    ids, cn = stream()
    if ("model", D) not in _cache:
        rng = np.random.default_rng(31)
        _cache[("model", D)] = tuple((rng.random((V, D)) - 0.5).astype(np.float32) for _ in range(2))
    u0, v0 = _cache[("model", D)]
    assert (np.abs(u0) < 0.5).all() and (np.abs(v0) < 0.5).all() and (u0 != 0).all() and (v0 != 0).all()
    t = w2b.Trainer(V, D, window, negative, bitlevel, num_threads=1, iter=1, alpha=0.0, sample=0.0, train_words=int(cn.sum()),
                    compute_loss=True, row_groups=True, atomic_rank_u=V - 1, refresh_rows_u=refresh)
    t.set_model(u0, v0)
    t.set_vocab_counts(cn, TABLE)
    t.set_corpus(ids)
    t.set_shards(np.zeros(1, np.int64))
    r = dict(name=t.worker_kernel_name(), u0=u0, v0=v0)
    r["loss"] = t.train_epoch(positions_per_launch=COPY_POSITIONS)
    fin, r["wca"], r["alpha"], _ = t.epoch_status()
    assert fin
    r["u"], r["v"] = t.get_model()
    t.close()
    _cache[key] = r
    return r


@pytest.mark.parametrize("D,window,negative,bitlevel,refresh", COPY_CASES)
def test_refreshed_copies_hold_their_master_rows(gpu, D, window, negative, bitlevel, refresh):
    """k_refresh_rows and the load at rc_copy[crow - 1].  With alpha = 0 no row moves, so a copy equals its master whenever
    it is read and the epoch loss is a pure function of which values were read: the run that reads rows 1 .. refresh_rows_u at
    their copies must book the loss of the run without copies EXACTLY (one worker: the same terms in the same lanes and
    order), where test_gpu_groups.py test_refreshed_copies_forced allows 1 % between racing workers.  A copy that holds
    another row, a refresher that skips rows (1, 3, 5: no multiple of the four rows a wavefront keeps in flight; 64: every
    row of the buffer), a copy read at the wrong index all change dot products of the hottest words -- at least 10 % of the
    positions are such words (asserted; tests/test_testlib_walk.py has the figures) and each is in most windows around it.
    Nothing reports whether a launch read its copies: while they are not filled yet the workers read the master rows, by
    design, so a launch that ended before the refresher's first sweep -- or a device on which the refresher's stream only
    runs after the workers' -- would pass here whatever the copies hold.  That these launches of 2000 positions do read
    them was shown once on an MI355X with a library whose refresher stored the NEGATED row into the copy: all six cases
    failed at the loss comparison.  (Likewise: staging zeros in the second trip of the context-row load turned the six wide-window
    cases above red and none of the twelve others; taking ar2 as 0 for added rows in phase C turned ten of the eleven -reg
    cases red -- every all-atomic one, the rank-25 one, and the "auto" ones whose hottest rows the plan adds.)"""
    base = frozen_run(D, window, negative, bitlevel, -1)
    got = frozen_run(D, window, negative, bitlevel, refresh)
    assert (base["name"], got["name"]) == ("groups", "groups")
    assert hot_share(refresh) >= 0.10
    for r in (base, got):
        assert np.array_equal(r["u"].view(np.uint32), r["u0"].view(np.uint32))
        assert np.array_equal(r["v"].view(np.uint32), r["v0"].view(np.uint32))
    assert got["wca"] == base["wca"] and got["alpha"] == base["alpha"]
    print("GROUPS copies D=%d refresh=%d: loss %.17g with, %.17g without" % (D, refresh, got["loss"], base["loss"]))
    assert base["loss"] < 0.0
    assert got["loss"] == base["loss"]
