"""Full-length beam search on the host: the library exports the new debug taps, the package lists
them, and the argument errors that need no engine are statuses.  An engine cannot be made without a GPU, so the option
full_beam and the refusals are asserted in tests/test_gpu_beam_full.py.  Without the feature the symbols do not exist.
CPU only."""
import ctypes

NEW_TAPS = ("wt_dbg_self_attention_long_gather", "wt_dbg_beam_full_step", "wt_dbg_beam_full_finalize")


def test_the_taps_are_exported_and_listed(pkg):
    L = pkg.lib()
    for name in NEW_TAPS:
        assert name in pkg.DEBUG_SYMBOLS and getattr(L, name)


def test_the_argument_record_has_the_headers_layout(pkg):
    # 14 int32 scalars, then 27 pointers (include/wt_debug.h: wt_dbg_beam_full_args)
    assert ctypes.sizeof(pkg.BeamFullArgs) == 14 * 4 + 27 * ctypes.sizeof(ctypes.c_void_p)
    assert pkg.BeamFullArgs.logits.offset == 56 and pkg.BeamFullArgs.out_sum.offset == 56 + 26 * 8


def test_a_null_engine_is_an_argument_error(pkg):
    L = pkg.lib()
    invalid = [k for k, v in pkg.STATUS_NAMES.items() if v == "WT_ERR_INVALID_ARG"][0]
    a = pkg.BeamFullArgs()
    assert L.wt_dbg_beam_full_step(None, ctypes.byref(a)) == invalid
    assert L.wt_dbg_beam_full_finalize(None, ctypes.byref(a)) == invalid
    assert L.wt_dbg_self_attention_long_gather(None, 1, 1, 32, 0, None, None, None, None, None) == invalid
