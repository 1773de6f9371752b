"""The per-clip-context and batched-seeking entry points on the host: the symbols are exported and
listed, and the argument errors that need no engine are statuses.  An engine cannot be made without a GPU (its constructor
opens the device), so the refusals wt_engine_set_contexts makes from its arguments — more than 64 clips, offsets that
decrease, more than 4096 ids for a clip, an id outside the vocabulary — are asserted in tests/test_gpu_ragged_context.py;
what is left for the host is the NULL handle.  Without the feature the symbols do not exist.  CPU only."""
import ctypes

NEW = ("wt_engine_set_contexts", "wt_transcribe_long_batch", "wt_last_file_text", "wt_last_window_files")
NEW_TAPS = ("wt_dbg_self_attention_long_ragged", "wt_dbg_self_attention_prefill_ragged", "wt_dbg_dec_ln_gemm_ragged",
            "wt_dbg_ragged_cap")


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
    offsets = (ctypes.c_int32 * 2)(0, 2)
    assert L.wt_engine_set_contexts(None, ids, offsets, 1) == invalid
    assert L.wt_engine_set_contexts(None, None, None, 0) == invalid
    assert L.wt_transcribe_long_batch(None, None, None, 1) == invalid
    n = ctypes.c_size_t(7)
    assert L.wt_last_file_text(None, 0, None, 0, ctypes.byref(n)) == invalid
    assert L.wt_last_window_files(None, None, 0) == -invalid
