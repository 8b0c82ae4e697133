"""ctypes mirror of the reference's evaluator program (ref src/compute-accuracy.c) over include/word2bits_eval.h.

    ev = Evaluator("vectors.bin", bitlevel=0, threshold=0)          # ref :77-112
    print(ev.transcript(open("questions-words.txt", "rb").read()).decode())   # ref :113-188, same bytes

    ev = Evaluator("vectors.w2bp", bits=True)                        # 1-bit model kept packed: the exact integer scan
    rows, scores = ev.neighbors([ev.lookup(b"KING")], 10)
    ev = Evaluator("vectors2.w2bp", codes=True)                      # 2-bit model kept packed: the i8 matrix-core scan
    rows, scores = ev.bag([3, 17, 4, 9, 9], [0, 2, 5], 10)           # two bags of rows pooled: nearest to each sum
    rows, scores = ev.vectors(hidden, 10)                            # float vectors [nq, size] of one's own: nearest to each
    rows, scores = ev.cosmul(b1, b2, b3, 10)                         # analogies by the multiplicative rule 3CosMul
    rank = ev.rank(b1, b2, b3, expected)                             # where the expected answer stands, however far down
    cls = ev.classes(500)                                            # word classes by k-means (word2vec's -classes)
    ev.set_docs(ids, offsets); docs, scores = ev.docs(qids, qoffsets, 10)   # corpus texts nearest to query texts (RWMD)
    cos = ev.pairs([3, 17, 4, 9, 9], [0, 1, 2, 3, 5])                # given pairs of words / bags: (3, 17) and ([4], [9, 9])
    r, rho = rank_correlation(gold, cos)                             # ... and their correlation with human scores

The exhaustive scan runs on the MI355X (w2b_kernels_eval.hip, w2b_kernels_evalbits.hip, w2b_kernels_evalcodes.hip,
w2b_kernels_evalbag.hip, w2b_kernels_evalvec.hip, w2b_kernels_evalcosmul.hip, w2b_kernels_evalclasses.hip,
w2b_kernels_evaldocs.hip, w2b_kernels_evalpairs.hip);
there is no CPU path in this module.
"""
import ctypes as C

import numpy as np

from . import _lib


class Evaluator:
    """`fused=True` reproduces the reference built with its own Makefile flags (FMA-contracted dot products),
    `fused=False` the -ffp-contract=off build; answers are identical to that build's, ties included.

    `bits=True` (1-bit models: a bitlevel-1 .w2bp, or a float file reduced to its signs) keeps the rows packed on the
    device and ranks by the exact integer score I (include/word2bits_eval.h, "bits mode"): rows with I > 0, I descending,
    equal I by ascending row, score = float32(I) / float32(size).  `bitlevel` and `fused` are ignored.

    `codes=True` (2-bit models: a bitlevel-2 .w2bp, or a float file reduced by the bitlevel-2 rule) keeps the rows packed
    and scores by exact integer dot products scaled by the rows' lengths in a fixed float32 sequence
    (include/word2bits_eval.h, "codes mode").  `bitlevel` and `fused` are ignored."""

    def __init__(self, path, bitlevel=0, threshold=0, fused=True, device=0, _handle=None, bits=False, codes=False):
        self._h = C.c_void_p()
        if bits and codes:
            raise ValueError("bits and codes are two modes: give one of them")
        self._L = _lib.lib()
        if _handle is not None:
            self._h = _handle
        elif bits:
            _lib.check(self._L.w2b_eval_load_bits(str(path).encode(), int(threshold), int(device), C.byref(self._h)))
        elif codes:
            _lib.check(self._L.w2b_eval_load_codes(str(path).encode(), int(threshold), int(device), C.byref(self._h)))
        else:
            _lib.check(self._L.w2b_eval_load(str(path).encode(), int(bitlevel), int(threshold), int(bool(fused)),
                                             int(device), C.byref(self._h)))
        self.words = int(self._L.w2b_eval_words(self._h))
        self.size = int(self._L.w2b_eval_size(self._h))
        self.is_bits = bool(self._L.w2b_eval_is_bits(self._h))
        self.is_codes = bool(self._L.w2b_eval_is_codes(self._h))

    @classmethod
    def from_trainer(cls, trainer, words, bitlevel=0, threshold=0, fused=True, bits=False, codes=False):
        """The evaluator on a live Trainer (no file round trip): what Evaluator(path) would hold after the trainer's
        vectors had been saved to `path` with binary=1.  `words` = the vocabulary (Corpus.words()).  `bits=True` (a
        bitlevel-1 trainer): what Evaluator(path, bits=True) would hold after the packed save; the rows are packed on
        the device.  `codes=True` (a bitlevel-2 trainer): the same for Evaluator(path, codes=True)."""
        if bits and codes:
            raise ValueError("bits and codes are two modes: give one of them")
        L = _lib.lib()
        arr = (C.c_char_p * len(words))(*[w if isinstance(w, bytes) else w.encode("latin1") for w in words])
        h = C.c_void_p()
        if bits:
            _lib.check(L.w2b_eval_bits_from_trainer(trainer._h, len(words), arr, int(threshold), C.byref(h)))
        elif codes:
            _lib.check(L.w2b_eval_codes_from_trainer(trainer._h, len(words), arr, int(threshold), C.byref(h)))
        else:
            _lib.check(L.w2b_eval_from_trainer(trainer._h, len(words), arr, int(bitlevel), int(threshold), int(bool(fused)),
                                               C.byref(h)))
        return cls(None, _handle=h)

    def close(self):
        if self._h:
            self._L.w2b_eval_free(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def word(self, row):
        return self._L.w2b_eval_word(self._h, int(row))

    def lookup(self, upper_word):
        """First row whose upper-cased word equals `upper_word` (bytes), or `words` (ref :140-145)."""
        return int(self._L.w2b_eval_lookup(self._h, bytes(upper_word)))

    def matrix(self):
        out = np.empty((self.words, self.size), np.float32)
        _lib.check(self._L.w2b_eval_get_matrix(self._h, out.ctypes.data_as(_lib.f32p)))
        return out

    def bits(self):
        """The packed rows of a bits handle: uint64 [words, ceil(size / 64)] in the .w2bp layout."""
        out = np.empty((self.words, (self.size + 63) // 64), np.uint64)
        _lib.check(self._L.w2b_eval_get_bits(self._h, out.ctypes.data_as(_lib.u64p)))
        return out

    def codes(self):
        """The packed rows of a codes handle: uint64 [words, 2 * ceil(size / 64)] in the .w2bp layout."""
        out = np.empty((self.words, 2 * ((self.size + 63) // 64)), np.uint64)
        _lib.check(self._L.w2b_eval_get_codes(self._h, out.ctypes.data_as(_lib.u64p)))
        return out

    def _scan(self, fn, rows, *k):
        """One batched query of the C ABI: int32 row arrays (and k) in, (rows, scores) of shape [nq] or [nq, k] out."""
        rows = [np.ascontiguousarray(x, np.int32) for x in rows]
        shape = (len(rows[0]),) + tuple(max(x, 0) for x in k)
        best, bestd = np.empty(shape, np.int32), np.empty(shape, np.float32)
        p = lambda a: a.ctypes.data_as(_lib.i32p)
        _lib.check(fn(self._h, shape[0], *map(p, rows), *k, p(best), bestd.ctypes.data_as(_lib.f32p)))
        return best, bestd

    def _text(self, fn, text, *k):
        """One text query of the C ABI: bytes in, the malloc'ed answer copied out and freed."""
        text = bytes(text)
        out, n = C.c_void_p(), C.c_int64()
        _lib.check(fn(self._h, text, len(text), *k, C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value)
        finally:
            self._L.w2b_eval_free_text(out)

    def top1(self, b1, b2, b3):
        """ref :155-177 for a batch: (best row or -1, its score) per question."""
        return self._scan(self._L.w2b_eval_top1, (b1, b2, b3))

    def topk(self, b1, b2, b3, k):
        """ref :155-177 with N = k: (rows int32 [nq, k], scores float32 [nq, k]) in the reference's order (score down,
        equal scores by ascending row); a list of fewer than k rows ends in row -1 / score 0.  1 <= k <= 64."""
        return self._scan(self._L.w2b_eval_topk, (b1, b2, b3), int(k))

    def cosmul(self, b1, b2, b3, k):
        """The analogy "b1 is to b2 as b3 is to ?" by the multiplicative rule 3CosMul (w2b_eval_cosmul; bits and codes
        handles): score = (u2 * u3) / (u1 + 1e-6) with the similarities shifted to [0, 1].  Returns (rows int32 [nq, k],
        scores float32 [nq, k]) in the order of topk; b1, b2, b3 are excluded from their question's answers."""
        return self._scan(self._L.w2b_eval_cosmul, (b1, b2, b3), int(k))

    def cosmul_text(self, queries, k):
        """stdout of `nearest FILE k ... bits|codes cosmul < queries` as bytes: every line is three words A B C."""
        return self._text(self._L.w2b_eval_cosmul_text, queries, int(k))

    def rank(self, b1, b2, b3, target, details=False):
        """The place of row target[q] in the complete answer list of the question (b1, b2, b3) (w2b_eval_rank; bits and codes
        handles, the additive rule): 1-based, 0 when the target is one of the question's rows or its score is not > 0.
        Returns int32 [nq], or with details=True (rank, tied, score): `tied` = other rows of the list with exactly the
        target's score, `score` = what topk reports for the target (0 without a rank)."""
        rows = [np.ascontiguousarray(x, np.int32).ravel() for x in (b1, b2, b3, target)]
        if len({len(x) for x in rows}) != 1:
            raise ValueError("b1, b2, b3 and target must have the same length")
        return self._rank(self._L.w2b_eval_rank, rows, details)

    def neighbor_rank(self, rows, target, details=False):
        """The place of target[q] among the neighbours of rows[q] (gensim's rank; closer_than is rank - 1 rows):
        rank(rows, rows, rows, target)."""
        rows = [np.ascontiguousarray(x, np.int32).ravel() for x in (rows, target)]
        if len(rows[0]) != len(rows[1]):
            raise ValueError("rows and target must have the same length")
        return self._rank(self._L.w2b_eval_neighbor_rank, rows, details)

    def _rank(self, fn, rows, details):
        n = len(rows[0])
        rank, tied, score = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        p = lambda a: a.ctypes.data_as(_lib.i32p)
        _lib.check(fn(self._h, n, *map(p, rows), p(rank), p(tied) if details else None,
                      score.ctypes.data_as(_lib.f32p) if details else None))
        return (rank, tied, score) if details else rank

    def rank_text(self, queries):
        """stdout of `nearest FILE k ... bits|codes rank < queries` as bytes: every line is two words A G or four A B C G."""
        return self._text(self._L.w2b_eval_rank_text, queries)

    def neighbors(self, rows, k):
        """The k nearest rows of each row in `rows` (the row itself excluded): topk(rows, rows, rows, k)."""
        return self._scan(self._L.w2b_eval_neighbors, (rows,), int(k))

    def combine(self, rows, signs, k):
        """The signed multi-word question (w2b_eval_combine): `rows` and `signs` are int arrays [nq, nt], nt <= 7, a sign
        is +1, -1 or 0 (slot unused, its row ignored).  Returns (rows int32 [nq, k], scores float32 [nq, k]) in the order
        of topk; every used row is excluded from its question's answers.  fp32 and bits handles."""
        rows, signs = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(signs, np.int8)
        if rows.ndim != 2 or rows.shape != signs.shape:
            raise ValueError("rows and signs must both be [nq, nt]")
        nq, nt = rows.shape
        k = int(k)
        best, bestd = np.empty((nq, max(k, 0)), np.int32), np.empty((nq, max(k, 0)), np.float32)
        _lib.check(self._L.w2b_eval_combine(self._h, nq, nt, rows.ctypes.data_as(_lib.i32p), signs.ctypes.data_as(_lib.i8p),
                                            k, best.ctypes.data_as(_lib.i32p), bestd.ctypes.data_as(_lib.f32p)))
        return best, bestd

    def most_similar(self, positive, negative, k):
        """gensim's most_similar for a batch: `positive` and `negative` are lists of row lists, one per question (either may
        be empty for a question, not both).  A question's slots are its positives, then its negatives, padded with sign 0."""
        if len(positive) != len(negative):
            raise ValueError("one list of positive and one of negative rows per question")
        nt = max([len(p) + len(n) for p, n in zip(positive, negative)] + [1])
        rows, signs = np.zeros((len(positive), nt), np.int32), np.zeros((len(positive), nt), np.int8)
        for q, (p, n) in enumerate(zip(positive, negative)):
            rows[q, :len(p) + len(n)] = list(p) + list(n)
            signs[q, :len(p)] = 1
            signs[q, len(p):len(p) + len(n)] = -1
        return self.combine(rows, signs, k)

    def combine_text(self, queries, k):
        """stdout of `nearest FILE k ... signed < queries` as bytes: every line is 1 to 7 tokens +WORD, -WORD or WORD."""
        return self._text(self._L.w2b_eval_combine_text, queries, int(k))

    def bag(self, ids, offsets, k, exclude_own=True):
        """The bag question (w2b_eval_bag; bits and codes handles): question q is the rows ids[offsets[q]:offsets[q + 1]]
        pooled into one integer vector -- any number of rows up to 4096, an id < 0 is padding, a repeated row adds.  Returns
        (rows int32 [nq, k], scores float32 [nq, k]) in the order of topk.  `exclude_own=True` keeps the bag's own rows out of
        its answers (as combine does); False asks for them too (the words nearest to a document, its own included)."""
        ids, offsets = np.ascontiguousarray(ids, np.int32).ravel(), np.ascontiguousarray(offsets, np.int64).ravel()
        nq, k = max(len(offsets) - 1, 0), int(k)
        best, bestd = np.empty((nq, max(k, 0)), np.int32), np.empty((nq, max(k, 0)), np.float32)
        _lib.check(self._L.w2b_eval_bag(self._h, len(ids), ids.ctypes.data_as(_lib.i32p), nq, offsets.ctypes.data_as(_lib.i64p),
                                        int(exclude_own), k, best.ctypes.data_as(_lib.i32p), bestd.ctypes.data_as(_lib.f32p)))
        return best, bestd

    def bag_text(self, queries, k, exclude_own=True):
        """stdout of `nearest FILE k ... bits|codes bag < queries` as bytes: every line is one bag of 1 to 4096 words."""
        return self._text(self._L.w2b_eval_bag_text, queries, int(exclude_own), int(k))

    def vectors(self, x, k, normalize=True):
        """The vector question (w2b_eval_vectors; every handle kind): `x` is float32 [nq, size] (or one vector [size]), vectors
        the caller computed itself.  Returns (rows int32 [nq, k], scores float32 [nq, k]) in the order of topk; nothing is
        excluded.  `normalize=True` scores by cosine (x scaled by 1 / |x|), False leaves x as it is.  Every value must be
        finite and 0 or of a magnitude in 2^-60 .. 2^60."""
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim == 1:
            x = x[None, :]
        if x.ndim != 2 or x.shape[1] != self.size:
            raise ValueError("x must be [nq, %d]" % self.size)
        nq, k = x.shape[0], int(k)
        best, bestd = np.empty((nq, max(k, 0)), np.int32), np.empty((nq, max(k, 0)), np.float32)
        _lib.check(self._L.w2b_eval_vectors(self._h, nq, x.ctypes.data_as(_lib.f32p), int(normalize), k,
                                            best.ctypes.data_as(_lib.i32p), bestd.ctypes.data_as(_lib.f32p)))
        return best, bestd

    def vectors_text(self, queries, k, normalize=True):
        """stdout of `nearest FILE k ... vector < queries` as bytes: every line is `size` numbers."""
        return self._text(self._L.w2b_eval_vectors_text, queries, int(normalize), int(k))

    def classes(self, n_classes, iters=10, init=None, details=False):
        """Word classes by k-means (w2b_eval_classes; bits and codes handles): at most `iters` iterations of spherical k-means
        on the packed rows, from `init` (int32 [words], classes in [0, n_classes)) or from class = row % n_classes.  Returns
        cls int32 [words]; with details=True (cls, score float32 [words], T int32 [n_classes, size] the classes' summed rows,
        counts int64 [n_classes], iters_run, moved)."""
        K = int(n_classes)
        cls, score = np.empty(self.words, np.int32), np.empty(self.words, np.float32)
        T, counts = np.empty((max(K, 0), self.size), np.int32), np.empty(max(K, 0), np.int64)
        it, moved = C.c_int32(), C.c_int64()
        if init is not None:
            init = np.ascontiguousarray(init, np.int32).ravel()
            if len(init) != self.words:
                raise ValueError("init must hold one class per row")
        _lib.check(self._L.w2b_eval_classes(self._h, K, int(iters), None if init is None else init.ctypes.data_as(_lib.i32p),
                                            cls.ctypes.data_as(_lib.i32p), score.ctypes.data_as(_lib.f32p),
                                            T.ctypes.data_as(_lib.i32p), counts.ctypes.data_as(_lib.i64p), C.byref(it),
                                            C.byref(moved)))
        return (cls, score, T, counts, it.value, moved.value) if details else cls

    def classes_text(self, n_classes, iters=10):
        """stdout of `classes FILE n_classes iters ... bits|codes` as bytes: one line "<word> <class>" per row (word2vec's
        -classes file)."""
        out, n = C.c_void_p(), C.c_int64()
        _lib.check(self._L.w2b_eval_classes_text(self._h, int(n_classes), int(iters), C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value)
        finally:
            self._L.w2b_eval_free_text(out)

    def classes_timing(self):
        """(assign ms, sums ms): the device time of the last classes() call, split into its assign scans and its sums passes."""
        a, s = C.c_double(), C.c_double()
        _lib.check(self._L.w2b_eval_classes_timing(self._h, C.byref(a), C.byref(s)))
        return a.value, s.value

    def set_docs(self, ids, offsets):
        """The corpus of the document question (w2b_eval_docs_set; bits and codes handles): document d is the rows
        ids[offsets[d]:offsets[d + 1]], at most 1024 positions, an id < 0 is padding.  Replaces an earlier corpus; an empty
        one (offsets == [0]) drops it."""
        ids, offsets = np.ascontiguousarray(ids, np.int32).ravel(), np.ascontiguousarray(offsets, np.int64).ravel()
        _lib.check(self._L.w2b_eval_docs_set(self._h, len(ids), ids.ctypes.data_as(_lib.i32p), max(len(offsets) - 1, 0),
                                             offsets.ctypes.data_as(_lib.i64p)))

    def set_docs_text(self, text):
        """The corpus from text (bytes): one document per line, empty lines included; words not in the vocabulary are
        dropped.  Returns (n_docs, dropped)."""
        text = bytes(text)
        n, dropped = C.c_int64(), C.c_int64()
        _lib.check(self._L.w2b_eval_docs_set_text(self._h, text, len(text), C.byref(n), C.byref(dropped)))
        return n.value, dropped.value

    def docs_count(self):
        return int(self._L.w2b_eval_docs_count(self._h))

    def docs(self, ids, offsets, k, symmetric=True, all_scores=False):
        """The document question (w2b_eval_docs): query q is the rows ids[offsets[q]:offsets[q + 1]]; the answer is the k
        documents of the corpus nearest to it by relaxed word mover's similarity -- every word matched to its best word of
        the other text, the matches averaged; symmetric=True takes the smaller of the two directions, False scores how well
        the query's words are matched in the document alone.  Returns (documents int32 [nq, k], scores float32 [nq, k]) in
        the order of topk, a short list ending in -1 / 0; with all_scores=True also every score, float32 [nq, n_docs]."""
        ids, offsets = np.ascontiguousarray(ids, np.int32).ravel(), np.ascontiguousarray(offsets, np.int64).ravel()
        nq, k = max(len(offsets) - 1, 0), int(k)
        best, bestd = np.empty((nq, max(k, 0)), np.int32), np.empty((nq, max(k, 0)), np.float32)
        every = np.empty((nq, self.docs_count()), np.float32) if all_scores else None
        _lib.check(self._L.w2b_eval_docs(self._h, len(ids), ids.ctypes.data_as(_lib.i32p), nq, offsets.ctypes.data_as(_lib.i64p),
                                         int(symmetric), k, best.ctypes.data_as(_lib.i32p), bestd.ctypes.data_as(_lib.f32p),
                                         every.ctypes.data_as(_lib.f32p) if all_scores else None))
        return (best, bestd, every) if all_scores else (best, bestd)

    def docs_text(self, queries, k, symmetric=True):
        """stdout of `nearest FILE k ... bits|codes docs CORPUS.txt < queries` as bytes: every line is one query text, an
        answer line is "<rank>\t<line number of the document>\t<score>"."""
        return self._text(self._L.w2b_eval_docs_text, queries, int(symmetric), int(k))

    def docs_timing(self):
        """(table ms, walk ms): the device time of the last docs() call, split into its pair-table phase and its walk."""
        a, s = C.c_double(), C.c_double()
        _lib.check(self._L.w2b_eval_docs_timing(self._h, C.byref(a), C.byref(s)))
        return a.value, s.value

    def pairs(self, ids, offsets, parts=False):
        """Pair similarity (w2b_eval_pairs; bits and codes handles): `offsets` has 2 * np + 1 entries, bag 2p of `ids` is side A
        of pair p and bag 2p + 1 side B; an id < 0 is padding, a repeated row adds.  Returns the cosines of the pooled integer
        vectors, float32 [np] (+0 for a pair with an empty side); with parts=True also int64 [np, 3] = J, N_A, N_B, the exact
        integers the score is built from."""
        ids, offsets = np.ascontiguousarray(ids, np.int32).ravel(), np.ascontiguousarray(offsets, np.int64).ravel()
        if len(offsets) % 2 != 1:
            raise ValueError("offsets must hold 2 * np + 1 entries")
        n = len(offsets) // 2
        score, triple = np.empty(n, np.float32), np.empty((n, 3), np.int64)
        _lib.check(self._L.w2b_eval_pairs(self._h, len(ids), ids.ctypes.data_as(_lib.i32p), n, offsets.ctypes.data_as(_lib.i64p),
                                          score.ctypes.data_as(_lib.f32p), triple.ctypes.data_as(_lib.i64p)))
        return (score, triple) if parts else score

    def similarity(self, a, b):
        """The cosine of two words or two bags (gensim's similarity / n_similarity): `a` and `b` are a row or a list of rows."""
        a, b = np.atleast_1d(np.asarray(a, np.int32)).ravel(), np.atleast_1d(np.asarray(b, np.int32)).ravel()
        return float(self.pairs(np.concatenate([a, b]), [0, len(a), len(a) + len(b)])[0])

    def pairs_text(self, text, details=True):
        """stdout of `similarity FILE ... bits|codes [summary] < text` as bytes: every line is "A <tab> B <tab> gold"; one line
        per pair (details=True), then the counts and Pearson's and Spearman's correlation with the gold column."""
        return self._text(self._L.w2b_eval_pairs_text, text, int(bool(details)))

    def nearest_text(self, queries, k):
        """stdout of `nearest FILE k < queries` as bytes: one word per line = its neighbours, three = an analogy."""
        return self._text(self._L.w2b_eval_nearest_text, queries, int(k))

    def set_topk_scratch(self, nbytes):
        """Upper bound for the device scratch of one top-k launch (0 = default); results never depend on it."""
        _lib.check(self._L.w2b_eval_set_topk_scratch(self._h, int(nbytes)))

    def transcript(self, questions, method="add"):
        """stdout of `compute_accuracy FILE bitlevel threshold < questions` as bytes.  method="cosmul" (bits and codes
        handles) answers every question by 3CosMul instead: `compute_accuracy FILE ... bits|codes cosmul`.  method="rank"
        (bits and codes handles) keeps the additive transcript and adds the lines that begin with RANKS (mean reciprocal
        rank, hits@1 / 5 / 10, unranked) after every "Total accuracy" line: `compute_accuracy FILE ... bits|codes rank`."""
        fns = {"add": self._L.w2b_eval_transcript, "cosmul": self._L.w2b_eval_transcript_cosmul,
               "rank": self._L.w2b_eval_transcript_rank}
        if method not in fns:
            raise ValueError('method must be "add", "cosmul" or "rank"')
        return self._text(fns[method], questions)

    def set_kernel(self, variant):
        """1 = f32 MFMA kernel (default), 0 = the same fused chain on the vector ALU (cross-check)"""
        _lib.check(self._L.w2b_eval_set_kernel(self._h, int(variant)))

    def timing(self):
        """(kernel ms, launches, multiply-adds) of the score kernel since the last call."""
        ms, n, macs = C.c_double(), C.c_int64(), C.c_double()
        _lib.check(self._L.w2b_eval_timing_read(self._h, C.byref(ms), C.byref(n), C.byref(macs)))
        return ms.value, n.value, macs.value


def rank_correlation(x, y):
    """(Pearson's r, Spearman's rho) of two equally long sequences (w2b_rank_correlation: double arithmetic on the host, ties
    share the mean of their ranks as in scipy's spearmanr); NaN with fewer than 2 values or a zero variance."""
    x, y = np.ascontiguousarray(x, np.float64).ravel(), np.ascontiguousarray(y, np.float64).ravel()
    if len(x) != len(y):
        raise ValueError("x and y must have the same length")
    r, rho = C.c_double(), C.c_double()
    _lib.check(_lib.lib().w2b_rank_correlation(len(x), x.ctypes.data_as(_lib.f64p), y.ctypes.data_as(_lib.f64p), C.byref(r),
                                               C.byref(rho)))
    return r.value, rho.value


def compute_accuracy(path, questions, bitlevel=0, threshold=0, fused=True, device=0):
    """The reference's `main` (ref :63-189) as a function: returns the stdout bytes."""
    ev = Evaluator(path, bitlevel, threshold, fused, device)
    try:
        return ev.transcript(questions)
    finally:
        ev.close()
