"""Pair similarity on the GPU (include/word2bits_eval.h, w2b_eval_pairs): both packed modes against the host twin -- the three
integers of every pair and the score bits, no tolerance anywhere; the bits one-word pairs against the neighbour scan; the
chunking, the refusals, the text form, the command line and the timing.

Shape: V = 300 rows.  Row lengths 1, 63, 64, 65 (a last word of one column), 200, 257 (five 64-column blocks, more than the long
path's workgroup has wavefronts: two block pairs and a last single block that holds one column) and 650 (eleven blocks: on the
long path wavefront 0 pools two block pairs, wavefront 1 a pair and the single last block).  Bag
lengths 0, 1, 2, 63, 64, 65 (the pooling takes ids in batches of 64), 1024, 1025, 4096.  The kernel's path boundaries
(w2b_kernels_evalpairs.hip), each with pairs on either side in the same batch:
  one-word path (both handle kinds): both bags exactly one id >= 0 -- beside [r, -1] / [c], [-1] / [c] and [] / [c] on the short path;
  short / long: a pair of 256 ids (128 + 128, 255 + 1) is the last one a single wavefront pools, 257 ids (128 + 129, 1 + 256)
  the first with a workgroup of its own;
  block pairs / a last single block: sizes with an even (65, 200: 2 and 4) and an odd (1, 63, 64: 1; 257: 5; 650: 11) number of
  blocks."""
import os
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import ROOT, write_vectors_file
from topk_testlib import same_floats, seeded_matrix
from cosmul_testlib import write_model
from pairs_testlib import MAX_BAG, flatten_pairs, host_pairs, make_model, standard_pairs

pytestmark = pytest.mark.gpu
SIM = os.path.join(ROOT, "similarity")
V = 300
SIZES = [1, 63, 64, 65, 200, 257, 650]
LENGTHS = [0, 1, 2, 63, 64, 65, 1024, 1025, 4096]
_cache = {}


def names_of(n):
    return [b"w%d" % i for i in range(n)]


def handle(tmp_path, bitlevel, packed, D):
    path = write_model(str(tmp_path / ("m%d.w2bp" % bitlevel)), bitlevel, names_of(packed.shape[0]), packed, D)
    return w2b.Evaluator(path, bits=bitlevel == 1, codes=bitlevel == 2), path


def batch(bitlevel, D):
    """the model, its pairs and the host twin's (score, parts) -- computed once, never changed"""
    if (bitlevel, D) not in _cache:
        rng = np.random.default_rng(3000 * D + bitlevel)
        M, packed = make_model(rng, bitlevel, V, D)
        pairs, named = standard_pairs(rng, V, LENGTHS, totals=(256,))
        ids, offsets = flatten_pairs(pairs)
        rc, score, parts = host_pairs(packed, D, bitlevel, ids, offsets)
        assert rc == 0
        for a in (packed, ids, offsets, score, parts):
            a.setflags(write=False)
        _cache[(bitlevel, D)] = (M, packed, pairs, named, ids, offsets, score, parts)
    return _cache[(bitlevel, D)]


@pytest.mark.parametrize("bitlevel", [1, 2])
@pytest.mark.parametrize("D", SIZES)
def test_parts_and_score_bits_equal_the_host_twin(gpu, D, bitlevel, tmp_path):
    M, packed, pairs, named, ids, offsets, want_score, want_parts = batch(bitlevel, D)
    sizes = np.diff(offsets)
    total = sizes[0::2] + sizes[1::2]
    assert {256, 257} <= set(total.tolist()) and total.max() == 2 * MAX_BAG          # both sides of the long-path boundary
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    assert ev.is_bits == (bitlevel == 1) and ev.is_codes == (bitlevel == 2)
    score, parts = ev.pairs(ids, offsets, parts=True)
    assert parts.dtype == np.int64 and parts.shape == (len(pairs), 3) and score.dtype == np.float32
    assert np.array_equal(parts, want_parts), np.argwhere(parts != want_parts)[:10]
    assert same_floats(score, want_score)
    assert same_floats(ev.pairs(ids, offsets), want_score)                          # the scores alone
    for name in ("identical", "identical_permuted", "identical_long", "one_word_same"):
        assert score[named[name]].view(np.uint32) == 0x3F800000, name
    for name in ("empty_no_ids", "empty_both", "empty_padding", "empty_cancels", "one_padding_word"):
        p = named[name]
        assert score[p].view(np.uint32) == 0 and (parts[p, 1] == 0 or parts[p, 2] == 0), name
    a, b = pairs[named["padding"]]
    assert ev.similarity(a, b) == float(want_score[named["padding"]])
    assert ev.similarity(11, 11) == 1.0 and ev.similarity(0, [1]) == -1.0
    ev.close()


@pytest.mark.parametrize("D", [63, 200, 257])
def test_bits_one_word_pairs_equal_the_neighbour_scores(gpu, D, tmp_path):
    M, packed = batch(1, D)[:2]
    ev, _ = handle(tmp_path, 1, packed, D)
    rng = np.random.default_rng(D)
    seen = 0
    for r in rng.integers(0, V, 6):
        rows, bestd = ev.neighbors([r], 64)
        cs = rows[0][rows[0] >= 0]
        seen += len(cs)
        ids = np.stack([np.full(len(cs), r, np.int32), cs.astype(np.int32)], axis=1).ravel()
        got = ev.pairs(ids, np.arange(2 * len(cs) + 1))
        assert same_floats(got, bestd[0][:len(cs)])
    assert seen > 64
    ev.close()


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_chunking_timing_and_refusals(gpu, bitlevel, tmp_path):
    D = 65
    M, packed, pairs, named, _, _, _, _ = batch(bitlevel, D)
    rng = np.random.default_rng(5)
    some = [pairs[i] for i in rng.permutation(len(pairs))]
    some = (some + some + some + some)[:200]
    ids, offsets = flatten_pairs(some)
    rc, want_score, want_parts = host_pairs(packed, D, bitlevel, ids, offsets)
    assert rc == 0
    ev, _ = handle(tmp_path, bitlevel, packed, D)
    ev.timing()
    score, parts = ev.pairs(ids, offsets, parts=True)
    ms, launches, macs = ev.timing()
    assert launches == 1 and ms > 0 and macs == float(len(ids)) * D
    assert np.array_equal(parts, want_parts) and same_floats(score, want_score)
    ev.set_topk_scratch(1)                                                # the smallest budget: 64 pairs per launch
    s2, p2 = ev.pairs(ids, offsets, parts=True)
    assert ev.timing()[1] == 4 >= 3
    assert np.array_equal(p2, parts) and same_floats(s2, score)
    ev.set_topk_scratch(0)
    assert same_floats(ev.pairs(ids, offsets), score)

    L = _lib.lib()
    out_s, out_p = np.full(2, -5.0, np.float32), np.full((2, 3), -5, np.int64)

    def raw(ids, off):
        ids, off = np.asarray(ids, np.int32), np.asarray(off, np.int64)
        return L.w2b_eval_pairs(ev._h, len(ids), ids.ctypes.data_as(_lib.i32p), len(off) // 2, off.ctypes.data_as(_lib.i64p),
                                out_s.ctypes.data_as(_lib.f32p), out_p.ctypes.data_as(_lib.i64p))

    assert raw([3, 4, 5, V], [0, 1, 2, 3, 4]) == _lib.W2B_EINVAL and b"pair 1: id out of range" in L.w2b_last_error()
    assert raw(np.zeros(MAX_BAG + 2, np.int32), [0, MAX_BAG + 1, MAX_BAG + 2]) == _lib.W2B_EINVAL
    assert b"a bag holds at most 4096 ids" in L.w2b_last_error()
    assert raw([1, 2], [0, 1, 1]) == _lib.W2B_EINVAL and b"offsets must start at 0" in L.w2b_last_error()
    assert np.all(out_s == -5.0) and np.all(out_p == -5)                   # refused: nothing written
    with pytest.raises(ValueError):
        ev.pairs([1, 2], [0, 1])
    assert ev.pairs([], [0]).shape == (0,)                                 # no pairs
    assert raw([3, 4, 5, V - 1], [0, 1, 2, 3, 4]) == _lib.W2B_OK           # a following valid call works
    rc, hs, hp = host_pairs(packed, D, bitlevel, [3, 4, 5, V - 1], [0, 1, 2, 3, 4])
    assert np.array_equal(out_p, hp) and same_floats(out_s, hs)
    ev.close()


def test_fp32_handle_refuses(gpu, tmp_path):
    rng = np.random.default_rng(8)
    path = write_vectors_file(str(tmp_path / "m.bin"), names_of(40), seeded_matrix(rng, "1bit", 40, 20))
    ev = w2b.Evaluator(path, 0, 0)
    for call in (lambda: ev.pairs([1, 2], [0, 1, 2]), lambda: ev.pairs_text(b"w1\tw2\t1\n"), lambda: ev.similarity(1, 2)):
        with pytest.raises(w2b.W2bError) as e:
            call()
        assert e.value.code == _lib.W2B_EINVAL
        assert "not available on an fp32 handle: load the file with bits or codes" in str(e.value)
    ev.close()


TEXT = (b"# word pairs, then sentences\n"
        b"w1\tw2\t3.5\n"
        b"w3 w4 7.25\n"
        b"\n"
        b"w5 nosuch w6\tw7 w8\t1e1\n"
        b"nosuch either\tw9\t2.0\n"
        b"w1\tw2\n"
        b"w1\tw2\tabc\n"
        b"  W10  \t w11 \t 0.5\r\n"
        b"w12 w13 w14 1\n"
        b"w1\t\t2\n"
        b"w2\tw1\tinf\n"
        b"   \n"
        b"w20\tw21\t-1")


@pytest.mark.parametrize("bitlevel", [1, 2])
def test_text_form_and_command_line(gpu, bitlevel, tmp_path):
    D = 65
    M, packed = batch(bitlevel, D)[:2]
    ev, path = handle(tmp_path, bitlevel, packed, D)
    scored = [([1], [2], 3.5), ([3], [4], 7.25), ([5, 6], [7, 8], 10.0), ([10], [11], 0.5), ([20], [21], -1.0)]
    s = [np.float32(ev.similarity(a, b)) for a, b, _ in scored]
    assert len(set(s)) > 1
    line = lambda i, gold, a, b: ("%.6f" % float(s[i])).encode() + b"\t" + gold + b"\t" + a + b"\t" + b + b"\n"
    r, rho = w2b.rank_correlation([g for _, _, g in scored], [float(x) for x in s])
    summary = (b"pairs: 5 scored, 1 skipped, 5 malformed\nwords: 16 looked up, 3 not in vocabulary\n" +
               ("pearson: %.6f\nspearman: %.6f\n" % (r, rho)).encode())
    details = (line(0, b"3.5", b"w1", b"w2") + line(1, b"7.25", b"w3", b"w4") + line(2, b"1e1", b"w5 nosuch w6", b"w7 w8") +
               b"skipped\t2.0\tnosuch either\tw9\n" + b"malformed line 7\nmalformed line 8\n" + line(3, b"0.5", b"W10", b"w11") +
               b"malformed line 10\nmalformed line 11\nmalformed line 12\n" + line(4, b"-1", b"w20", b"w21"))
    assert ev.pairs_text(TEXT) == details + summary
    assert ev.pairs_text(TEXT, details=False) == summary
    assert ev.pairs_text(b"") == b"pairs: 0 scored, 0 skipped, 0 malformed\nwords: 0 looked up, 0 not in vocabulary\n" \
                                  b"pearson: nan\nspearman: nan\n"
    mode = "bits" if bitlevel == 1 else "codes"
    for args, want in (([path, mode], details + summary), ([path, "0", mode, "summary"], summary),
                       ([path, mode, "summary"], summary)):
        r = subprocess.run([SIM] + args, input=TEXT, capture_output=True, timeout=300)
        assert r.returncode == 0 and r.stdout == want, (args, r.stderr)
    assert subprocess.run([SIM, path, "fast"], input=b"", capture_output=True, timeout=300).returncode == 2
    ev.close()
