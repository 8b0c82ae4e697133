"""The text forms of the evaluator (include/word2bits_eval.h), the part that needs no GPU: with a NULL handle every entry point
refuses with W2B_EINVAL, and which message it gives pins the order of its checks -- what needs no handle is refused before
the handle is looked at, except where the form has always refused the handle first."""
import ctypes as C

import pytest

from word2bits_amd import _lib


def text_call(name, *args):
    """name(NULL, b"a", 1, *args, &out, &len) -> (rc, message, out)"""
    L = _lib.lib()
    out, n = C.c_void_p(), C.c_int64()
    rc = getattr(L, name)(None, b"a", 1, *args, C.byref(out), C.byref(n))
    return rc, L.w2b_last_error(), out.value


# (entry point, its arguments between the text and the outputs, the message)
CASES = [
    ("w2b_eval_nearest_text", (0,), b"bad argument"),                       # k = 0: the handle is refused first
    ("w2b_eval_cosmul_text", (0,), b"k must be 1..64"),
    ("w2b_eval_cosmul_text", (1,), b"null handle"),
    ("w2b_eval_combine_text", (0,), b"bad argument"),
    ("w2b_eval_bag_text", (0, 0), b"bad argument"),                         # exclude_own, k
    ("w2b_eval_vectors_text", (2, 1), b"normalize must be 0 or 1"),         # normalize, k
    ("w2b_eval_vectors_text", (0, 1), b"null handle"),
    ("w2b_eval_docs_text", (2, 1), b"symmetric must be 0 or 1"),            # symmetric, k
    ("w2b_eval_docs_text", (0, 1), b"null handle"),
]


@pytest.mark.parametrize("name,args,message", CASES, ids=["-".join([c[0][9:]] + [str(a) for a in c[1]]) for c in CASES])
def test_null_handle_refusal_order(name, args, message):
    rc, err, out = text_call(name, *args)
    assert rc == _lib.W2B_EINVAL
    assert name.encode() + b": " + message in err, err
    assert out is None


def test_docs_set_text_refusal_order():
    L = _lib.lib()
    n_docs, dropped = C.c_int64(-7), C.c_int64(-7)
    assert L.w2b_eval_docs_set_text(None, b"a", -1, C.byref(n_docs), C.byref(dropped)) == _lib.W2B_EINVAL
    assert b"w2b_eval_docs_set_text: bad argument" in L.w2b_last_error(), L.w2b_last_error()
    assert L.w2b_eval_docs_set_text(None, b"a", 1, C.byref(n_docs), C.byref(dropped)) == _lib.W2B_EINVAL
    assert b"w2b_eval_docs_set_text: null handle" in L.w2b_last_error(), L.w2b_last_error()
    assert n_docs.value == -7 and dropped.value == -7
