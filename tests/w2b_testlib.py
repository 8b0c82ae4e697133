"""Shared helpers for the test-suite (test infrastructure only).

* ctypes binding of the CPU oracle (oracle/libw2b_oracle.so) -- the checker.
* deterministic synthetic corpora (no network: text8 is not available offline).
* a runner for the unmodified reference binaries under oracle/_ref/ (compiled by
  oracle/Makefile from /root/reference when that mount exists).
"""
import ctypes as C
import os
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
REF_DIR = os.path.join(ORACLE_DIR, "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")

c_f32p = C.POINTER(C.c_float)
c_i32p = C.POINTER(C.c_int)
c_i64p = C.POINTER(C.c_longlong)


def fptr(a):
    return a.ctypes.data_as(c_f32p)


def iptr(a):
    return a.ctypes.data_as(c_i32p)


def lptr(a):
    return a.ctypes.data_as(c_i64p)


class OracleModel(C.Structure):
    _fields_ = [
        ("vocab_size", C.c_longlong), ("dim", C.c_longlong), ("train_words", C.c_longlong),
        ("iter", C.c_longlong),
        ("window", C.c_int), ("negative", C.c_int), ("bitlevel", C.c_int), ("num_threads", C.c_int),
        ("starting_alpha", C.c_float), ("sample", C.c_float), ("reg", C.c_float),
        ("cn", c_i64p), ("u", c_f32p), ("v", c_f32p), ("exp_table", c_f32p),
        ("table", c_i32p), ("table_size", C.c_longlong),
        ("alpha", C.c_float), ("word_count_actual", C.c_longlong), ("compute_loss", C.c_int),
    ]


_oracle = {}


def build_oracle(fma=False):
    name = "libw2b_oracle_fma.so" if fma else "libw2b_oracle.so"
    so = os.path.join(ORACLE_DIR, name)
    src = os.path.join(ORACLE_DIR, "w2b_oracle.c")
    if (not os.path.exists(so)) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", ORACLE_DIR, name], stdout=subprocess.DEVNULL)
    return so


def oracle(fma=False):
    """ctypes handle of the CPU oracle (built on demand with gcc).  fma=True: the same source
    compiled with FMA contraction -- a second legitimate build used only as a drift yardstick."""
    if fma in _oracle:
        return _oracle[fma]
    L = C.CDLL(build_oracle(fma))
    L.w2bo_quantize.restype = C.c_float
    L.w2bo_quantize.argtypes = [C.c_float, C.c_int]
    L.w2bo_quantize_array.argtypes = [c_f32p, c_f32p, C.c_longlong, C.c_int]
    L.w2bo_sigmoid.restype = C.c_float
    L.w2bo_sigmoid.argtypes = [C.c_float]
    L.w2bo_build_exp_table.argtypes = [c_f32p]
    L.w2bo_lcg_next.restype = C.c_uint64
    L.w2bo_lcg_next.argtypes = [C.c_uint64]
    L.w2bo_exp_index.restype = C.c_int
    L.w2bo_exp_index.argtypes = [C.c_float]
    L.w2bo_init_net.argtypes = [C.c_longlong, C.c_longlong, c_f32p, c_f32p]
    L.w2bo_build_unigram_table.argtypes = [c_i64p, C.c_longlong, c_i32p, C.c_longlong]
    L.w2bo_keep_prob.restype = C.c_float
    L.w2bo_keep_prob.argtypes = [C.c_longlong, C.c_float, C.c_longlong]
    L.w2bo_center_update.restype = C.c_double
    L.w2bo_center_update.argtypes = [C.POINTER(OracleModel), c_i32p, C.c_int, c_i32p, c_i32p, C.c_int,
                                     C.c_float, c_f32p]
    L.w2bo_reg_terms.restype = C.c_double
    L.w2bo_reg_terms.argtypes = [C.c_int]
    L.w2bo_train_tuples.restype = C.c_double
    L.w2bo_train_tuples.argtypes = [C.POINTER(OracleModel), C.c_longlong, c_i32p, c_i32p, c_i32p, c_i32p,
                                    C.c_float]
    L.w2bo_train_worker_tokens.restype = C.c_double
    L.w2bo_train_worker_tokens.argtypes = [C.POINTER(OracleModel), C.c_longlong, c_i32p, C.c_longlong,
                                           C.c_longlong, C.c_int]
    L.w2bo_train_epoch_tokens.restype = C.c_double
    L.w2bo_train_epoch_tokens.argtypes = [C.POINTER(OracleModel), c_i32p, C.c_longlong, c_i64p, c_i32p,
                                          C.c_int]
    L.w2bo_vocab_learn.restype = C.c_void_p
    L.w2bo_vocab_learn.argtypes = [C.c_char_p, C.c_int]
    L.w2bo_vocab_learn_ex.restype = C.c_void_p
    L.w2bo_vocab_learn_ex.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.w2bo_vocab_free.argtypes = [C.c_void_p]
    for f in ("w2bo_vocab_size", "w2bo_vocab_train_words", "w2bo_vocab_file_size"):
        getattr(L, f).restype = C.c_longlong
        getattr(L, f).argtypes = [C.c_void_p]
    L.w2bo_vocab_word.restype = C.c_char_p
    L.w2bo_vocab_word.argtypes = [C.c_void_p, C.c_longlong]
    L.w2bo_vocab_count.restype = C.c_longlong
    L.w2bo_vocab_count.argtypes = [C.c_void_p, C.c_longlong]
    L.w2bo_vocab_search.restype = C.c_int
    L.w2bo_vocab_search.argtypes = [C.c_void_p, C.c_char_p]
    L.w2bo_tokenize_file.restype = C.c_longlong
    L.w2bo_tokenize_file.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(c_i32p), C.POINTER(c_i64p)]
    L.w2bo_shard_start.restype = C.c_longlong
    L.w2bo_shard_start.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong, c_i64p, C.c_longlong, c_i32p]
    L.w2bo_run.restype = C.c_int
    L.w2bo_run.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                           C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_double)]
    L.w2bo_run_ex.restype = C.c_int
    L.w2bo_run_ex.argtypes = L.w2bo_run.argtypes + [C.c_int]
    _oracle[fma] = L
    return L


class OracleState:
    """Convenience owner of an oracle model (numpy-backed buffers)."""

    def __init__(self, cn, dim, window=5, negative=5, bitlevel=1, num_threads=1, iters=1, alpha=0.05,
                 sample=1e-3, reg=0.0, table_size=100000, compute_loss=1, init=True, fma=False):
        L = oracle(fma)
        self.L = L
        self.cn = np.ascontiguousarray(cn, dtype=np.int64)
        V = len(self.cn)
        self.V, self.D = V, dim
        self.u = np.zeros((V, dim), np.float32)
        self.v = np.zeros((V, dim), np.float32)
        if init:
            L.w2bo_init_net(V, dim, fptr(self.u), fptr(self.v))
        self.exp_table = np.zeros(1001, np.float32)
        L.w2bo_build_exp_table(fptr(self.exp_table))
        self.table = np.zeros(table_size, np.int32)
        if negative > 0:
            L.w2bo_build_unigram_table(lptr(self.cn), V, iptr(self.table), table_size)
        m = OracleModel()
        m.vocab_size, m.dim, m.train_words, m.iter = V, dim, int(self.cn.sum()), iters
        m.window, m.negative, m.bitlevel, m.num_threads = window, negative, bitlevel, num_threads
        m.starting_alpha, m.sample, m.reg = alpha, sample, reg
        m.cn, m.u, m.v = lptr(self.cn), fptr(self.u), fptr(self.v)
        m.exp_table, m.table, m.table_size = fptr(self.exp_table), iptr(self.table), table_size
        m.alpha, m.word_count_actual, m.compute_loss = alpha, 0, compute_loss
        self.m = m

    def train_tuples(self, center, ctx_off, ctx, neg, alpha):
        center = np.ascontiguousarray(center, np.int32)
        ctx_off = np.ascontiguousarray(ctx_off, np.int32)
        ctx = np.ascontiguousarray(ctx, np.int32)
        neg = np.ascontiguousarray(neg, np.int32)
        return self.L.w2bo_train_tuples(C.byref(self.m), len(center), iptr(center), iptr(ctx_off),
                                        iptr(ctx), iptr(neg), alpha)

    def train_epoch_tokens(self, ids, starts, overrides=None):
        ids = np.ascontiguousarray(ids, np.int32)
        starts = np.ascontiguousarray(starts, np.int64)
        ov = None if overrides is None else np.ascontiguousarray(overrides, np.int32)
        self.L.w2bo_reg_terms(1)
        loss = self.L.w2bo_train_epoch_tokens(C.byref(self.m), iptr(ids), len(ids), lptr(starts),
                                              None if ov is None else iptr(ov), len(starts))
        self.reg_terms = self.L.w2bo_reg_terms(1)      # of this epoch, one worker only: what -reg booked into `loss`
        return loss


# ----------------------------------------------------------------------------- what a worker visits

def walk(ids, cn, window, negative, sample, table_size=50000, max_sentence=1000, dup_words=None):
    """Host restatement of what ONE reference worker (thread id 0) visits on a token stream (ref :368-509: sub-sampling,
    window draw, negative draws -- the LCG ledger, no arithmetic on rows).  Returns (positions trained, positions whose
    context list holds a word twice, context rows visited, target rows visited).  `dup_words`, a dict, is filled with
    {word: positions whose context list holds THAT word more than once} -- which rows the order-dependent update of
    ref :494-503 really meets."""
    L = oracle()
    cn = np.ascontiguousarray(cn, np.int64)
    tw, nv = int(cn.sum()), len(cn)
    table = np.zeros(table_size, np.int32)
    if negative > 0:
        L.w2bo_build_unigram_table(lptr(cn), nv, iptr(table), table_size)
    table = table.tolist()
    keep = [float(L.w2bo_keep_prob(int(c), sample, tw)) if sample > 0 else 2.0 for c in cn.tolist()]
    toks = ids.tolist()
    A, Cc, M = 25214903917, 11, (1 << 64) - 1
    rng, pos, n = 0, 0, len(toks)
    sen, spos = [], 0
    trained = dups = rows_u = rows_v = 0
    while True:
        if not sen:
            eof = False
            while True:
                if pos >= n:
                    eof = True
                    break
                w = toks[pos]
                pos += 1
                if w == 0:
                    break
                if sample > 0:
                    rng = (rng * A + Cc) & M
                    if keep[w] < (rng & 0xFFFF) / 65536.0:
                        continue
                sen.append(w)
                if len(sen) >= max_sentence:
                    break
            spos = 0
            if eof:
                break
        rng = (rng * A + Cc) & M
        b = rng % window
        word = sen[spos] if sen else 0
        ctx = [sen[c] for c in range(spos - window + b, spos + window - b + 1) if c != spos and 0 <= c < len(sen)]
        if ctx:
            nt = 1
            for _ in range(negative):
                rng = (rng * A + Cc) & M
                t = table[(rng >> 16) % table_size]
                if t == 0:
                    t = rng % (nv - 1) + 1
                nt += t != word
            trained += 1
            dups += len(set(ctx)) < len(ctx)
            if dup_words is not None and len(set(ctx)) < len(ctx):
                for w in {w for w in ctx if ctx.count(w) > 1}:
                    dup_words[w] = dup_words.get(w, 0) + 1
            rows_u += len(ctx)
            rows_v += nt
        spos += 1
        if spos >= len(sen):
            sen = []
    return trained, dups, rows_u, rows_v


def row_sumsq_floor(bitlevel, *tables):
    """smallest sum of q^2 over a row (row 0, "</s>", is never visited) among the given tables"""
    L = oracle()
    lo = np.inf
    for tab in tables:
        x = np.ascontiguousarray(tab[1:], np.float32)
        q = np.empty_like(x)
        L.w2bo_quantize_array(fptr(x), fptr(q), x.size, bitlevel)
        lo = min(lo, float((q.astype(np.float64) ** 2).sum(axis=1).min()))
    return lo


# ----------------------------------------------------------------------------- corpora

def zipf_ids(rng, vocab, n, s=1.0):
    """ids in [1, vocab) with P(k) ~ 1/k^s (rank 1 most frequent)."""
    w = 1.0 / np.arange(1, vocab, dtype=np.float64) ** s
    cdf = np.cumsum(w)
    cdf /= cdf[-1]
    return (np.searchsorted(cdf, rng.random(n)) + 1).astype(np.int64)


def write_corpus(path, seed=0, vocab=300, n_tokens=5000, line_len=40, quirks=True):
    """A small whitespace-separated corpus of tokens 'w<id>' with the tokenizer's corner cases:
    tabs, CRs, empty lines, a very long line (> MAX_SENTENCE_LENGTH tokens), no trailing newline."""
    rng = np.random.default_rng(seed)
    ids = zipf_ids(rng, vocab, n_tokens)
    out = []
    i = 0
    line = 0
    while i < n_tokens:
        if quirks and line == 3:
            ln = 1300                      # > 1000-token sentence chunking (ref :410)
        elif quirks and line == 5:
            ln = 0                         # empty line -> bare </s> (ref :145-147)
        else:
            ln = int(rng.integers(1, 2 * line_len))
        toks = ["w%d" % t for t in ids[i:i + ln]]
        i += ln
        sep = "\t" if (quirks and line % 7 == 2) else " "
        s = sep.join(toks)
        if quirks and line % 5 == 1:
            s = "  " + s + " \r"
        out.append(s)
        line += 1
    text = "\n".join(out)                  # no trailing newline: last token dropped (ref :135-138)
    with open(path, "w") as f:
        f.write(text)
    return path


# ----------------------------------------------------------------------------- reference binaries

def ref_binary(name):
    p = os.path.join(REF_DIR, name)
    return p if os.path.exists(p) else None


LIVE_REF_JSON = os.path.join(GOLDEN, "live_reference.json")


def sha256(data):
    import hashlib
    return hashlib.sha256(data).hexdigest()


def reference_sha(key, inputs, produce):
    """sha256 of what the unmodified reference program writes for one test case.

    `inputs` are the bytes that determine the case (files, flags, stdin); `produce()` runs the live binary and returns
    its output bytes, or None where oracle/_ref/ is not built.  Live runs are checked against the recording in
    tests/golden/live_reference.json (W2B_RECORD_LIVE_REF=1 rewrites it from them); without the binary the recording
    stands in, for exactly the inputs it was made from."""
    import json
    rec = json.load(open(LIVE_REF_JSON)) if os.path.exists(LIVE_REF_JSON) else {}
    live = produce()
    if live is not None:
        entry = {"inputs": sha256(inputs), "output": sha256(live)}
        if os.environ.get("W2B_RECORD_LIVE_REF") == "1":
            rec[key] = entry
            with open(LIVE_REF_JSON, "w") as f:
                json.dump(rec, f, indent=0, sort_keys=True)
                f.write("\n")
        elif rec.get(key, {}).get("inputs") == entry["inputs"]:
            assert rec[key]["output"] == entry["output"], "live reference differs from its recording: %s" % key
        return entry["output"]
    assert key in rec, "no recorded reference output for %s (oracle/_ref/ not built here)" % key
    assert rec[key]["inputs"] == sha256(inputs), "inputs of %s differ from the recorded ones" % key
    return rec[key]["output"]


def run_ref(name, train, output, **kw):
    """Run oracle/_ref/<name> with word2bits flags; returns stdout."""
    exe = ref_binary(name)
    assert exe, "oracle/_ref/%s not built (make -C oracle ref needs /root/reference)" % name
    args = [exe, "-train", train, "-output", output]
    for k, v in kw.items():
        args += ["-" + k.replace("_", "-"), str(v)]
    return subprocess.run(args, check=True, capture_output=True, text=True).stdout


def read_vectors(path, binary):
    """Parse a word2bits output file (ref :560-576) -> (words, float32 matrix)."""
    with open(path, "rb") as f:
        data = f.read()
    nl = data.index(b"\n")
    V, D = (int(x) for x in data[:nl].split())
    pos = nl + 1
    words, M = [], np.zeros((V, D), np.float32)
    for a in range(V):
        sp = data.index(b" ", pos)
        words.append(data[pos:sp].decode("latin1"))
        pos = sp + 1
        if binary:
            M[a] = np.frombuffer(data, dtype="<f4", count=D, offset=pos)
            pos += 4 * D
        else:
            nl2 = data.index(b"\n", pos)
            M[a] = np.array(data[pos:nl2].split(), dtype=np.float64).astype(np.float32)
            pos = nl2
        assert data[pos:pos + 1] == b"\n"
        pos += 1
    return words, M


def eval_oracle():
    """oracle/eval_oracle.py (the CPU restatement of the reference evaluator) as a module; builds the C part."""
    import importlib.util
    build_oracle()
    spec = importlib.util.spec_from_file_location("eval_oracle", os.path.join(ORACLE_DIR, "eval_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_vectors_file(path, names, M):
    """the binary writer's format (ref src/word2bits.cpp:560-576): 'V D\\n', then 'word ' + D float32 + '\\n'."""
    with open(path, "wb") as f:
        f.write(b"%d %d\n" % M.shape)
        for n, row in zip(names, M):
            f.write(n + b" " + np.asarray(row, "<f4").tobytes() + b"\n")
    return path


def write_disjoint_shard_corpus(path, n_shards=4, sentences=60, vocab_per_shard=40, seed=0, prefix=b""):
    """A corpus on which a MULTI-THREADED run of the reference is deterministic, so that the per-thread logic
    (fseek offsets ref :377, quotas :414-421, seeds :368, the sentence that crosses the quota being read but not
    trained) can be compared bit for bit: `n_shards` byte-identical-length shards, each with its own vocabulary
    (fixed-width words), boundaries on sentence boundaries, every shard well under the 10000 words after which a
    thread would touch the shared alpha (:379-393).  Train it with -threads n_shards -negative 0: then no two
    threads ever touch the same row.  `prefix` (e.g. b"zz zz\\n") shifts the thread offsets into the middle of
    words."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 30, sentences)
    shards = []
    for k in range(n_shards):
        letter = "abcdefghijklmnop"[k]
        words = rng.integers(0, vocab_per_shard, int(lens.sum()))
        out, i = [], 0
        for ln in lens:
            out.append(" ".join("%s%02d" % (letter, w) for w in words[i:i + ln]))
            i += ln
        shards.append(("\n".join(out) + "\n").encode())
    assert len({len(s) for s in shards}) == 1
    with open(path, "wb") as f:
        f.write(prefix + b"".join(shards))
    return path


# Held-out regimes of the Hogwild fidelity gates (round 4): shapes and distributions that no knob of the library was ever
# swept on -- the rules that pick hot rows / lossless rows from the word counts must carry over to them unchanged.
HELDOUT = {
    # a mid-sized vocabulary, short window, few negatives, one bit, no sub-sampling (every word kept by -min-count 5)
    "heldout_k5": dict(corpus=dict(vocab=100_000, n_tokens=8_000_000, s=1.0, every=5, seed=41),
                       flags=dict(bitlevel=1, size=300, window=5, negative=5, iter=1, sample=0)),
    # a steeper distribution (Zipf exponent 1.2) at the BASELINE configs[2] shape, the reference's default sub-sampling
    "heldout_zipf12": dict(corpus=dict(vocab=70_000, n_tokens=6_000_000, s=1.2, every=0, seed=42),
                           flags=dict(bitlevel=2, size=400, window=8, negative=24, iter=2)),
}


# The first held-out regime again, long enough (60 M tokens) for `-threads 0` to fill the device: the one setting in which the
# library gives the hottest rows per-XCD copies -- a balance measured on the benchmarked regime, checked
# here on a regime it was never measured on.  One reference run at 256 threads (4.5 minutes of the host) is its band.
HELDOUT_BIG = {
    "heldout_k5_big": dict(corpus=dict(vocab=100_000, n_tokens=60_000_000, s=1.0, every=5, seed=43),
                           flags=dict(bitlevel=1, size=300, window=5, negative=5, iter=1, sample=0)),
    # round 6 (asked for by the round-5 review, recorded BEFORE any constant of the full-device mode was touched again): a second
    # held-out full-device long-stream regime -- a vocabulary of a million words, a steeper distribution, another row length,
    # window and number of negatives than anything the merge period / weight / number of copies were ever measured on
    "heldout_v1m": dict(corpus=dict(vocab=1_000_000, n_tokens=80_000_000, s=1.1, every=5, seed=44),
                        flags=dict(bitlevel=1, size=512, window=5, negative=10, iter=1, sample=0)),
    # round 6 (review, weak 1d): the row lengths at which the row-group kernel is the automatic choice (BASELINE configs[0] /
    # configs[2]) on a LONG stream -- 100 M tokens over the text8-sized vocabulary, the reference's default sub-sampling;
    # round 5 had only ever checked that kernel on corpora of at most 17 M tokens
    "long_d200": dict(corpus=dict(vocab=70_000, n_tokens=100_000_000, s=1.0, every=0, seed=45),
                      flags=dict(bitlevel=1, size=200, window=8, negative=24, iter=1)),
    "long_d400b2": dict(corpus=dict(vocab=70_000, n_tokens=100_000_000, s=1.0, every=0, seed=45),
                        flags=dict(bitlevel=2, size=400, window=8, negative=24, iter=1)),
}


def write_heldout_corpus(path, name):
    c = (HELDOUT.get(name) or HELDOUT_BIG[name])["corpus"]
    return write_zipf_text_corpus(path, vocab=c["vocab"], n_tokens=c["n_tokens"], seed=c["seed"], s=c["s"], every=c["every"])


def write_zipf_text_corpus(path, vocab=70000, n_tokens=17_000_000, seed=0, line=1000, s=1.0, every=0):
    """A text8-SIZED stand-in (text8 itself is not available offline): n_tokens Zipf(1) draws over `vocab` words
    'w<id>', one line of `line` tokens each (text8 is a single line; the reference cuts sentences at 1000 tokens
    anyway, ref :410).  Deterministic for a given numpy version; used by the fidelity tests and by the script that
    records what the unmodified reference does on the same file (tests/golden/make_fidelity_bands.py)."""
    rng = np.random.default_rng(seed)
    ids = zipf_ids(rng, vocab, n_tokens, s)
    if every:                          # (s, every: the held-out regimes; the defaults write the round-3 file byte for byte)
        base = np.repeat(np.arange(1, vocab, dtype=np.int64), every)
        rng.shuffle(base)
        ids = np.concatenate([base, ids])
    words = np.array([b"w%d" % i for i in range(vocab)], dtype=object)
    with open(path, "wb") as f:
        for o in range(0, len(ids), line):
            f.write(b" ".join(words[ids[o:o + line]]))
            f.write(b"\n")
    return path


def write_headline_corpus(path, vocab=400_000, n_zipf=20_000_000, seed=1234, line=1000):
    """BASELINE configs[1] as a text file (SURVEY 8d "CPU baseline" recipe): every one of the vocab-1 words five times
    (so that -min-count 5 keeps all `vocab` rows), shuffled, followed by n_zipf Zipf(1) draws; a newline every `line`
    tokens.  Deterministic for a given numpy version.  Used by tests/golden/make_fidelity_bands.py (what the unmodified
    reference does on it) and by the fidelity test of the benchmarked regime."""
    rng = np.random.default_rng(seed)
    base = np.repeat(np.arange(1, vocab, dtype=np.int64), 5)
    rng.shuffle(base)
    ids = np.concatenate([base, zipf_ids(rng, vocab, n_zipf)])
    words = np.array([b"w%d" % i for i in range(vocab)], dtype=object)
    with open(path, "wb") as f:
        for o in range(0, len(ids), line):
            f.write(b" ".join(words[ids[o:o + line]]))
            f.write(b"\n")
    return path


def write_reduce_vocab_corpus(path, kind, seed=0):
    """Corpora on which ReduceVocab (ref :245-263) runs when vocab_hash_size is 3000 (more than 2100 words in the
    table, ref :293).  Generated with the reference's LCG in pure Python integers, so the bytes do not depend on the
    numpy version (tests/golden/reduce_vocab.json holds what the reference does on exactly these bytes).
      "zipf": 30 000 log-uniform draws over 6000 words, a newline every 50 tokens -- several reductions, "</s>" survives;
      "wipe": 2300 words that occur once and no newline first -- the first reduction empties the whole table, "</s>"
              included (the reference does not protect it), then 20 000 draws over 5000 words with newlines: another
              word ends up owning row 0 (and ends sentences), "</s>" comes back as an ordinary word."""
    x = 20240924 + seed          # seed 0 = the corpora of the committed fixture

    def draw():
        nonlocal x
        x = (x * 25214903917 + 11) & 0xFFFFFFFFFFFFFFFF
        return (x >> 16) & 0xFFFFF

    out = []
    if kind == "wipe":
        out.append(" ".join("u%d" % i for i in range(2300)) + " ")
        n, vocab, line = 20000, 5000, 40
    else:
        n, vocab, line = 30000, 6000, 50
    toks = ["w%d" % int(vocab ** (draw() / float(1 << 20))) for _ in range(n)]
    for o in range(0, n, line):
        out.append(" ".join(toks[o:o + line]) + "\n")
    with open(path, "w") as f:
        f.write("".join(out))
    return path
