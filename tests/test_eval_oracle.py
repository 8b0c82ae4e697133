"""not gpu: the evaluator oracle (oracle/eval_oracle.py + w2bo_eval_* in oracle/w2b_oracle.c) against the
committed stdout of BOTH builds of the unmodified reference evaluator (tests/golden/eval_golden.json, made by
tests/golden/make_eval_golden.py), and against runs of those builds on fresh random inputs: live where oracle/_ref/ is
built, else their recorded stdout (sha256 in tests/golden/live_reference.json).  Also the no-GPU behaviour of the
product evaluator."""
import json
import os
import subprocess

import numpy as np
import pytest

import word2bits_amd as w2b
from word2bits_amd import _lib
from w2b_testlib import GOLDEN, ROOT, eval_oracle, ref_binary, reference_sha, sha256, write_vectors_file

ALL = json.load(open(os.path.join(GOLDEN, "eval_golden.json")))
RUNS = [g for g in ALL if "vectors" in g]


def reference_stdout_sha(key, build, vec, args, q):
    """sha256 of the stdout of `<build> vec args < q`: the live binary where it is built, else its recording"""
    exe = ref_binary(build)

    def produce():
        return subprocess.run([exe, vec] + args, input=q, capture_output=True).stdout if exe else None
    inputs = open(vec, "rb").read() + repr((build, args)).encode() + b"\0" + q
    return reference_sha(key or "%s:%s" % (build, sha256(inputs)), inputs, produce)


def test_golden_set_is_discriminating():
    """the fixture must separate the two arithmetic modes and contain right and wrong answers"""
    by = {}
    for g in RUNS:
        by.setdefault((g["vectors"], g["bitlevel"], g["threshold"], g["questions"]), {})[g["build"]] = g["stdout"]
    assert sum(len(set(v.values())) == 2 for v in by.values()) >= 2
    assert any("ACCURACY TOP1: 4" in g["stdout"] for g in RUNS) and any("-nan" in g["stdout"] for g in RUNS)


@pytest.mark.parametrize("build", ["compute_accuracy", "compute_accuracy_nofma"])
def test_oracle_reproduces_reference_transcripts(build):
    E = eval_oracle()
    models = {}
    n = 0
    for g in RUNS:
        if g["build"] != build:
            continue
        key = (g["vectors"], g["bitlevel"], g["threshold"])
        if key not in models:
            models[key] = E.EvalModel(os.path.join(GOLDEN, g["vectors"]), g["bitlevel"], g["threshold"],
                                      fma=(build == "compute_accuracy"))
        got = E.transcript(models[key], open(os.path.join(GOLDEN, g["questions"]), "rb").read())
        assert got.decode("latin1") == g["stdout"], (g["vectors"], g["bitlevel"], g["threshold"], g["questions"])
        n += 1
    assert n == 24


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_matches_live_reference_on_fresh_inputs(seed, tmp_path):
    E = eval_oracle()
    rng = np.random.default_rng(seed)
    V, D = 180, (16, 21)[seed - 1]
    names = [b"</s>"] + [("w%d" % i).encode() for i in range(1, V)]
    M = (rng.integers(0, 2, (V, D)) * 2 - 1).astype(np.float32) / np.float32(3) if seed == 1 \
        else rng.standard_normal((V, D)).astype(np.float32)
    vec = write_vectors_file(str(tmp_path / "v.bin"), names, M)
    lines = []
    for s in range(7):
        lines.append(": s%d" % s)
        for _ in range(30):
            lines.append(" ".join("w%d" % i for i in rng.integers(1, V + 8, 4)))
    q = ("\n".join(lines) + "\n").encode()
    for build, fma in (("compute_accuracy", True), ("compute_accuracy_nofma", False)):
        want = reference_stdout_sha("eval_fresh_inputs[%d-%s]" % (seed, build), build, vec, ["0", "0"], q)
        got = E.transcript(E.EvalModel(vec, 0, 0, fma=fma), q)
        assert sha256(got) == want


@pytest.mark.parametrize("cut", ["in_name", "after_name", "float_boundary", "partial_float", "row_end"])
def test_oracle_matches_live_reference_on_truncated_files(cut, tmp_path):
    """a vector file that ends early (ref :96-105 keeps reading: EOF bytes become names, fread comes up short)"""
    E = eval_oracle()
    rng = np.random.default_rng(5)
    V, D = 30, 6
    names = [b"</s>"] + [("w%d" % i).encode() for i in range(1, V)]
    M = rng.standard_normal((V, D)).astype(np.float32)
    vec = write_vectors_file(str(tmp_path / "v.bin"), names, M)
    data = open(vec, "rb").read()
    row20 = data.index(b"w20 ")
    end = {"in_name": row20 + 2, "after_name": row20 + 4, "float_boundary": row20 + 4 + 8,
           "partial_float": row20 + 4 + 10, "row_end": row20 + 4 + 4 * D}[cut]
    open(vec, "wb").write(data[:end])
    # questions only over rows that were read completely (the cut row's values are indeterminate in the reference)
    q = (": s\n" + "".join("w%d w%d w%d w%d\n" % tuple(rng.integers(1, 20, 4)) for _ in range(40))).encode()
    want = reference_stdout_sha("eval_truncated[%s]" % cut, "compute_accuracy", vec, ["0", "20"], q)
    got = E.transcript(E.EvalModel(vec, 0, 20, fma=True), q)
    assert sha256(got) == want
    # the names the reader leaves behind for the rows after the cut
    m = E.EvalModel(vec, 0, 0, fma=True)
    assert m.words == V and m.names[19] == b"W19" and all(n == b"" for n in m.names[22:])


def test_product_evaluator_has_no_cpu_fallback():
    if w2b.lib().w2b_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(w2b.W2bError) as e:
        w2b.Evaluator(os.path.join(GOLDEN, "eval_1bit.bin"))
    assert e.value.code == _lib.W2B_ENOGPU
    with pytest.raises(w2b.W2bError) as e:
        w2b.Evaluator(os.path.join(GOLDEN, "no_such_file.bin"))
    assert e.value.code == _lib.W2B_EIO


def test_cli_usage_and_missing_file_match_reference():
    cli = os.path.join(ROOT, "compute_accuracy")
    want = {g["cli"]: g for g in ALL if g.get("cli") and g["build"] == "compute_accuracy"}
    r = subprocess.run([cli], capture_output=True)
    assert (r.stdout.decode(), r.returncode) == (want["usage"]["stdout"], want["usage"]["returncode"])
    r = subprocess.run([cli, os.path.join(GOLDEN, "no_such_file.bin")], capture_output=True, stdin=subprocess.DEVNULL)
    assert (r.stdout.decode(), r.returncode) == (want["notfound"]["stdout"], want["notfound"]["returncode"])


def test_oracle_question_loop_matches_live_reference_fuzz(tmp_path):
    """random token soups through the reference's scanf loop (ref :113-188) vs the oracle's restatement of it:
    section markers anywhere, EXIT, unknown words, truncated questions, missing trailing white space"""
    from hypothesis import given, settings, strategies as st
    E = eval_oracle()
    rng = np.random.default_rng(77)
    names = [b"</s>"] + [n.encode() for n in ("aa ab ac ad ba bb bc bd ca cb cc cd da db dc dd The the THE exit "
                                              "x1 x2 x3 x4 x5 x6 x7 x8 x9 y1 y2 y3 y4 y5 y6 y7 y8 y9 zz").split()]
    M = (rng.integers(0, 2, (len(names), 12)) * 2 - 1).astype(np.float32) / np.float32(3)
    vec = write_vectors_file(str(tmp_path / "v.bin"), names, M)
    om = E.EvalModel(vec, 0, 0, fma=False)
    words = [n.decode() for n in names[1:24]] + [":", ":", "EXIT", "exit", "nope", "Aa", "BB"]
    seps = [" ", " ", "\n", "\n", "\t", "  ", "\r\n", " \n "]

    # derandomize: the same examples on every run of one hypothesis version.  Where oracle/_ref/ is not built, each
    # example is looked up in tests/golden/live_reference.json by its inputs, recorded with hypothesis 6.164.0; another
    # version draws other examples and fails on "no recorded reference output" -- record again (W2B_RECORD_LIVE_REF=1)
    # where the reference binaries are built.
    @settings(max_examples=120, deadline=None, derandomize=True, database=None)
    @given(st.lists(st.tuples(st.sampled_from(words), st.sampled_from(seps)), min_size=0, max_size=60), st.booleans())
    def run(tokens, trailing):
        text = "".join(w + s for w, s in tokens)
        if not trailing:
            text = text.rstrip()
        q = text.encode()
        want = reference_stdout_sha(None, "compute_accuracy_nofma", vec, ["0", "0"], q)
        assert sha256(E.transcript(om, q)) == want, text

    run()


def test_oracle_vector_reader_matches_live_reference_fuzz(tmp_path):
    """random vector files through the reference's reader (ref :85-112) vs the oracle's restatement, observed through
    the transcript of a question stream that asks for every name: names with embedded newlines / tabs, mixed case,
    more than 50 characters, bytes >= 0x80, duplicates, header variants, -threshold"""
    from hypothesis import given, settings, strategies as st
    E = eval_oracle()
    name_st = st.lists(st.sampled_from(list("abAB\n\t_") + ["\xe9", "x" * 26]), min_size=1, max_size=4).map("".join)

    # (recordings keyed by the examples of hypothesis 6.164.0, as in the fuzz test above)
    @settings(max_examples=60, deadline=None, derandomize=True, database=None)
    @given(st.lists(name_st, min_size=2, max_size=9), st.integers(1, 5), st.integers(0, 12),
           st.sampled_from(["%d %d\n", "%d  %d\n", " %d\n%d\n"]), st.integers(0, 3))
    def run(names, D, threshold, header, seed):
        rng = np.random.default_rng(seed)
        V = len(names)
        # The reference's name array is `words * 50` bytes and its reader writes a terminating 0 at index 50 of a row
        # whose name has 50 or more characters (ref :99-104): in the LAST loaded row that is a heap overflow
        # (undefined behaviour -- the stock build dies after "Starting eval...").  Keep the last loaded row short
        # here; the long-last-row case is pinned oracle-only in test_oracle_long_name_in_last_row below.
        last = (min(V, threshold) if threshold else V) - 1
        names = list(names)
        if len(names[last].replace("\n", "")) >= 50:
            names[last] = names[last].replace("\n", "")[:49]
        M = rng.standard_normal((V, D)).astype(np.float32)
        p = str(tmp_path / "v.bin")
        with open(p, "wb") as f:
            f.write((header % (V, D)).encode())
            for n, row in zip(names, M):
                f.write(n.encode("latin1") + b" " + row.tobytes() + b"\n")
        asks = [n.replace("\n", "") for n in names] + ["ab", "AB", "x" * 50, "x" * 52]
        q = ": all\n" + "".join("%s %s %s %s\n" % (a, b, a, b) for a in asks for b in asks[:3]
                                if a.split() == [a] and b.split() == [b])
        q = q.encode("latin1")
        want = reference_stdout_sha(None, "compute_accuracy", p, ["0", str(threshold)], q)
        assert sha256(E.transcript(E.EvalModel(p, 0, threshold, fma=True), q)) == want, (names, D, threshold)

    run()


def test_oracle_long_name_in_last_row(tmp_path):
    """A name of 50+ characters in the LAST row drives the reference into a one-byte heap overflow (ref :99-104: the
    terminating 0 lands one byte past its `words * 50` name array), so there is no reference behaviour to match.  The
    restatement (and the product, tests/test_gpu_eval.py::test_vector_file_reader_fuzz) define it as a flat array
    with one spare byte: the name is its first 50 characters.  (In any other row the same name runs on into the next
    row's name -- that quirk IS reference behaviour and is pinned by the live fuzz above.)"""
    E = eval_oracle()
    names = ["</s>", "ab", "cd", "x" * 52]
    M = np.random.default_rng(5).standard_normal((4, 3)).astype(np.float32)
    p = str(tmp_path / "v.bin")
    with open(p, "wb") as f:
        f.write(b"4 3\n")
        for n, row in zip(names, M):
            f.write(n.encode() + b" " + row.tobytes() + b"\n")
    m = E.EvalModel(p, 0, 0, fma=True)
    assert m.names == [b"</S>", b"AB", b"CD", b"X" * 50]
    q = (": s\nab cd ab cd\n%s ab %s ab\n%s ab %s ab\n" % ("x" * 50, "x" * 50, "x" * 52, "x" * 52)).encode()
    out = E.transcript(m, q).decode()
    # the 50-character spelling is found (questions 1 and 2 are seen), the 52-character one is not
    assert out.endswith("Questions seen / total: 2 3   66.67 % \n") or out.rstrip().endswith("Questions seen / total: 2 3   66.67 %")
