"""The logit-suppression entry points on the host: the symbols are exported and listed, and the
argument errors that need no engine are statuses.  An engine cannot be made without a GPU (its constructor opens the
device), so the refusals wt_engine_set_suppress makes from its arguments — an id outside the vocabulary, EOT on the
always-list, more than 1024 ids — are asserted in tests/test_gpu_suppress.py; what is left for the host is the NULL handle
and wt_vocab_default_suppress, which needs no GPU at all.  Without the feature the symbols do not exist.  CPU only."""
import ctypes

NEW = ("wt_engine_set_suppress", "wt_vocab_default_suppress")
NEW_TAPS = ("wt_dbg_suppress_logits",)


def test_the_symbols_are_exported_and_listed(pkg):
    L = pkg.lib()
    for name in NEW:
        assert name in pkg.CAPI_SYMBOLS and getattr(L, name)
    for name in NEW_TAPS:
        assert name in pkg.DEBUG_SYMBOLS and getattr(L, name)


def test_a_null_engine_is_an_argument_error(pkg):
    L = pkg.lib()
    invalid = [k for k, v in pkg.STATUS_NAMES.items() if v == "WT_ERR_INVALID_ARG"][0]
    ids = (ctypes.c_int64 * 2)(1, 2)
    assert L.wt_engine_set_suppress(None, ids, 2, ids, 1) == invalid
    assert L.wt_engine_set_suppress(None, None, 0, None, 0) == invalid
    z = (ctypes.c_float * 8)()
    assert L.wt_dbg_suppress_logits(None, 1, 8, 8, z, z, ids, 1, None, 0, 0) == invalid
    v = ctypes.c_long(0)
    assert L.wt_engine_get_option(None, b"suppress_ids", ctypes.byref(v)) == invalid
    assert L.wt_engine_set_option(None, b"suppress_default", 1) == invalid


def test_default_suppress_argument_errors(pkg, assets):
    L = pkg.lib()
    invalid = [k for k, v in pkg.STATUS_NAMES.items() if v == "WT_ERR_INVALID_ARG"][0]
    n, nf = ctypes.c_int32(0), ctypes.c_int32(0)
    ids = (ctypes.c_int64 * 1024)()
    assert L.wt_vocab_default_suppress(None, ids, 1024, ctypes.byref(n), ids, 1024, ctypes.byref(nf)) == invalid
    v = pkg.Vocab(assets("micro")[1], True)
    assert L.wt_vocab_default_suppress(v._v, ids, 1024, None, ids, 1024, ctypes.byref(nf)) == invalid
    assert L.wt_vocab_default_suppress(v._v, ids, 1024, ctypes.byref(n), ids, 1024, None) == invalid
    assert L.wt_vocab_default_suppress(v._v, None, 5, ctypes.byref(n), ids, 1024, ctypes.byref(nf)) == invalid
    assert L.wt_vocab_default_suppress(v._v, ids, -1, ctypes.byref(n), ids, 1024, ctypes.byref(nf)) == invalid
    a, f = v.default_suppress()
    info = v.info()
    # the synthetic vocabulary: the single-byte tokens of the printable ASCII symbols and the special ids; it has no
    # bare-space token, so the first-list is EOT alone
    assert {info[k] for k in ("sot", "prev", "solm", "translate", "transcribe")} <= set(a) and info["eot"] not in a
    # Whisper's six special ids of the multilingual vocabulary: sot, translate, transcribe, startoflm, startofprev, nospeech
    assert [int(i) for i in a if i > info["eot"]] == [50258, 50358, 50359, 50360, 50361, 50362]
    assert list(f) == [info["eot"]] and ord("(") in a and ord("~") in a and ord("-") not in a and ord("A") not in a
    assert list(a) == sorted(set(a)) and len(a) <= 1024
    v.close()
