"""What the option full_bf16_all can show without a GPU: the four new debug taps are declared in
include/wt_debug.h and exported by the built library, and the float32 emulation of the bf16 score product in
tests/align_bf16_ref.py stays under a quarter of the kernel test's bar against float64 on the same rounded operands,
on the kernel test's own shapes — so the bar of tests/test_gpu_align_scores_bf16.py is reachable by its reference.  The
derivation of that bar (tests/test_gpu_align_kernels.py) carries over: bf16 x bf16 products are exact in fp32, and one
product per 32 columns accumulates no more error than three.  Without the feature the taps do not exist.  CPU only."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import align_bf16_ref as ab  # noqa: E402
from decoder_attn_ref import bf16_round  # noqa: E402

NEW_TAPS = ("wt_dbg_self_attention_long_ragged_bf16", "wt_dbg_self_attention_prefill_ragged_bf16", "wt_dbg_align_scores_bf16",
            "wt_dbg_f32_to_bf16")


def test_the_taps_are_declared_exported_and_listed(pkg):
    with open(os.path.join(ROOT, "include", "wt_debug.h")) as f:
        header = f.read()
    L = pkg.lib()
    for name in NEW_TAPS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in pkg.DEBUG_SYMBOLS and getattr(L, name)
    invalid = [k for k, v in pkg.STATUS_NAMES.items() if v == "WT_ERR_INVALID_ARG"][0]
    assert L.wt_dbg_self_attention_long_ragged_bf16(None, 1, 1, 32, 0, None, None, None, None, None, 32) == invalid
    assert L.wt_dbg_self_attention_prefill_ragged_bf16(None, 1, 1, 32, 0, 1, None, None, None, None, None, 32) == invalid
    assert L.wt_dbg_align_scores_bf16(None, 1, 2, 100, 1, 0, None, None, 1, None, None, 1, None, 1, 100, None, 1) == invalid
    assert L.wt_dbg_f32_to_bf16(None, 4, 0, None, None) == invalid


worst = {"rel": 0.0}


def _check(H, B, T, n_pos, F):
    qp, E = ab.case(H, B, T, n_pos, ab.seed_of(H, B, n_pos, T))
    d = 64 * H
    assert np.array_equal(bf16_round(E).reshape(E.shape), E)  # the cases hold bf16 values
    for b in range(B):
        for h in sorted({0, H - 1}):
            want = ab.softmax2(ab.scores64(qp, E, b, h), F[b])
            got = ab.softmax2(ab.scores_emulated(qp, E, b, h), F[b])
            rel, small = ab.relative_error(got, want)
            worst["rel"] = max(worst["rel"], rel)
            assert rel < ab.W_BOUND / 4 and small < 1e-29, (H, B, T, n_pos, b, h, rel, d)


@pytest.mark.parametrize("H,B,pos0,n_pos", ab.SHAPES)
def test_the_emulated_product_meets_a_quarter_of_the_bar(H, B, pos0, n_pos):
    _check(H, B, ab.T_SHORT, n_pos, ab.frames(B, ab.T_SHORT))


def test_the_emulated_product_at_the_full_length():
    H, B, _, n_pos = ab.LONG_SHAPE
    _check(H, B, ab.T_LONG, n_pos, np.array([1500, 205], np.int32))
    print(f"float32 emulation of the bf16 score product against float64: largest relative error {worst['rel']:.3g} "
          f"(a quarter of the bar: {ab.W_BOUND / 4:.3g})")
