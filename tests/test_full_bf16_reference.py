"""CPU: full-length decoding in the bf16 storage mode (option full_bf16).  The debug taps of the
three bf16 kernels are declared and exported (without the feature they are not), and the float64 reference the GPU
tests hold those kernels to is itself held against a plain float32 emulation at a quarter of the bar, at the key counts
the long kernels add to the 31-position chain's: a correct fp32 kernel can meet 1e-5 over 448 bf16-rounded keys."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decoder_attn_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402

TAPS = ["wt_dbg_self_attention_long_bf16", "wt_dbg_self_attention_long_gather_bf16", "wt_dbg_self_attention_prefill_bf16"]


def test_the_bf16_taps_are_declared_and_exported(pkg):
    txt = open(os.path.join(ROOT, "include", "wt_debug.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = pkg.lib()
    for tap in TAPS:
        assert re.search(r"\bint\s+" + tap + r"\s*\(", txt), f"{tap} is not declared in include/wt_debug.h"
        assert tap in pkg.DEBUG_SYMBOLS
        assert hasattr(L, tap), f"{tap} is not exported by the built library"
    # the signatures are those of the fp32 counterparts
    for tap in TAPS:
        assert getattr(L, tap).argtypes == getattr(L, tap[:-len("_bf16")]).argtypes


@pytest.mark.parametrize("H", [2, 6])
@pytest.mark.parametrize("keys", [33, 65, 448])
def test_a_float32_emulation_meets_a_quarter_of_the_bar(keys, H):
    """One new position over keys - 1 bf16-rounded cached rows, standard-normal operands: plain float32 arithmetic on
    the rounded operands stays within SELF_BAR / 4 of self_ref(.., bf16=True), and the caches are the roundings."""
    rng = np.random.default_rng(keys * 10 + H)
    B, d, pos = 3, 64 * H, keys - 1
    kc = np.zeros((B, keys, d), np.float32)
    vc = np.zeros((B, keys, d), np.float32)
    kc[:, :pos] = R.bf16_round(rng.standard_normal((B, pos, d)).astype(np.float32))
    vc[:, :pos] = R.bf16_round(rng.standard_normal((B, pos, d)).astype(np.float32))
    qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
    res = R.Emu().dbg_self_attention(qkv, kc, vc, pos, 1, bf16=True)
    ratio = R.check_self(res, qkv, kc, vc, pos, 1, True, margin=0.25, what=f"keys {keys} H {H}")
    print(f"keys {keys} H {H}: worst error / bar = {ratio:.3f}")
