"""GPU (-m gpu): the decoder attention of the 31-position chain, kernel by kernel, through the debug taps
of include/wt_debug.h: self_attention_step<BF> (A), cross_attention_step<NQ, DM, BF> through its per-chunk records (B) and
the kProCombine prologue of dec_gemm on hand-made records (C).  The cases, the float64 references and the bars live in
tests/decoder_attn_ref.py; tests/test_decoder_attention_reference.py runs the same cases on a plain float32 emulation
at a quarter of the bars.  Every test prints its worst measured error over bar."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decoder_attn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
INVALID, FORMAT = "WT_ERR_INVALID_ARG", "WT_ERR_FORMAT"


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def report(name, ratio):
    print(f"\n[decoder attention] {name}: worst error / bar = {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------- A. self_attention_step ---
@FORMS
@pytest.mark.parametrize("H", [2, 6, 8])
def test_a1_every_position(eng, H, bf16):
    """positions 0..31, one per launch, chained through the returned cache: after every launch the cache is the expected
    one bit for bit (the appended row, or its bf16 rounding, and nothing else) and the output within 1e-5 of float64"""
    report(f"A1 H={H} bf16={bf16}", R.a1_every_position(eng, H, bf16))


@FORMS
@pytest.mark.parametrize("pos0,npos,B,H", R.A2_GROUPS)
def test_a2_prompt_groups(eng, pos0, npos, B, H, bf16):
    """prompt groups at both ends of the 32 staged rows, up to the contract's limit (0, 32)"""
    report(f"A2 ({pos0},{npos}) bf16={bf16}", R.a2_prompt_group(eng, pos0, npos, B, H, bf16))


@FORMS
@pytest.mark.parametrize("B,pos0,npos", R.A3_WIDTHS)
def test_a3_chain_widths(eng, B, pos0, npos, bf16):
    """rows at the chain's width, every row checked: a wrong p * B + b shows"""
    report(f"A3 B={B} npos={npos} bf16={bf16}", R.a3_chain_width(eng, B, pos0, npos, bf16))


@FORMS
@pytest.mark.parametrize("cap", R.A4_CAPS)
def test_a4_cache_stride_and_stale_rows(eng, cap, bf16):
    """the b * cap * d stride of the full-length chain's cache, and NaN in every row at or behind the new positions: the
    outputs are finite and right, the NaN rows come back bit-identical"""
    report(f"A4 cap={cap} bf16={bf16}", R.a4_stride_and_stale_rows(eng, cap, bf16))


@FORMS
def test_a5_bit_identity_across_batches(eng, bf16):
    report(f"A5 bf16={bf16}", R.a5_bit_identity(eng, bf16))


@FORMS
@pytest.mark.parametrize("regime", R.A6_REGIMES)
def test_a6_softmax_regimes(eng, regime, bf16):
    """one key dominating by more than 200 (key 0, 15, 30, the new position), q = 0, all scores shifted by 32768, scores
    spread over +-50; the last two under the bar widened by 2 ds max|v|"""
    report(f"A6 {regime} bf16={bf16}", R.a6_softmax_regime(eng, regime, bf16))


@FORMS
def test_a7_refusals(pkg, eng, bf16):
    """what launch_self_attention refuses on the host, and an ordinary call afterwards"""
    rng = np.random.default_rng(700)
    B, H, d = 3, 2, 128
    qkv = rng.standard_normal((4 * B, 3 * d)).astype(np.float32)

    def refused(cap, pos, npos, **kw):
        c = np.zeros((B, cap, d), np.float32)
        with pytest.raises(pkg.WtError) as e:
            eng.dbg_self_attention(qkv, c, c, pos, npos, bf16=bf16, **kw)
        assert str(e.value).split(":")[0] == INVALID, (cap, pos, npos, kw)

    refused(32, -1, 1)
    refused(32, 0, 0)
    refused(32, 0, -1)
    refused(32, 32, 1)
    refused(32, 29, 4)
    refused(64, 32, 1)
    refused(448, 30, 3)
    refused(16, 14, 3)
    refused(16, 16, 1)
    refused(32, 3, 1, batch=0)
    refused(32, 3, 1, batch=-2)
    refused(32, 3, 1, heads=0)
    refused(32, 3, 1, heads=-1)
    report(f"A7 bf16={bf16}", R.a2_prompt_group(eng, 28, 4, 5, 6, bf16))


# ------------------------------------------------------------------------------------ B. cross_attention_step ---
@FORMS
@pytest.mark.parametrize("H", [2, 6, 8])
@pytest.mark.parametrize("nq", [1, 2, 3, 4])
def test_b1_every_instantiation(eng, nq, H, bf16):
    report(f"B1 nq={nq} H={H} bf16={bf16}", R.b1_instantiation(eng, nq, H, bf16))


@FORMS
def test_b2_chunk_geometry(eng, bf16):
    """T on the load-round edges x chunks in {1, 2, 4, 8}, empty chunks included; records and the combined output"""
    report(f"B2 bf16={bf16}", R.b2_geometry(eng, bf16))


@FORMS
def test_b2_full_length(eng, bf16):
    report(f"B2 T=1500 bf16={bf16}", R.b2_full_length(eng, bf16))


@FORMS
def test_b3_masked_past_keys(eng, bf16):
    report(f"B3 bf16={bf16}", R.b3_masked_past_keys(eng, bf16))


@FORMS
def test_b4_layernorm_inside(eng, bf16):
    report(f"B4 bf16={bf16}", R.b4_layernorm_inside(eng, bf16))


@FORMS
@pytest.mark.parametrize("regime,T,at", R.B5_CASES)
def test_b5_softmax_regimes(eng, regime, T, at, bf16):
    report(f"B5 {regime} T={T} at={at} bf16={bf16}", R.b5_softmax_regime(eng, regime, T, at, bf16))


@FORMS
def test_b6_bit_identity_and_grouping(eng, bf16):
    """a clip alone and in a batch of 32: the same records bit for bit; one nq = 4 launch and four nq = 1 launches each
    meet the float64 bars (their difference is printed, not asserted); a launch of a sub-range of positions leaves every
    other record's guard pattern untouched"""
    worst, diff = R.b6_bit_identity_and_grouping(eng, bf16)
    print(f"\n[decoder attention] B6 bf16={bf16}: largest difference nq = 4 against 4 x nq = 1: {diff:.3e}")
    report(f"B6 bf16={bf16}", worst)


@FORMS
def test_b7_refusals(pkg, eng, bf16):
    """what launch_cross_attention refuses on the host (nothing is allocated or launched), and an ordinary call afterwards"""
    rng = np.random.default_rng(7700)
    inp = R.cross_inputs(rng, 2, 2, 9, 5, bf16)

    def refused(code, chunks, nq, n_rows=None, inputs=inp, **kw):
        with pytest.raises(pkg.WtError) as e:
            eng.dbg_cross_attention_records(*inputs, chunks, nq, bf16=bf16, n_rows=n_rows, **kw)
        assert str(e.value).split(":")[0] == code, (chunks, nq, n_rows, kw)

    refused(INVALID, 0, 1)
    refused(INVALID, -1, 1)
    refused(INVALID, 10, 1)          # chunks > T
    refused(INVALID, 2, 5, n_rows=0)
    refused(INVALID, 2, 5, n_rows=5)
    refused(INVALID, 2, 1, batch=0)
    refused(INVALID, 2, 1, batch=-1)
    refused(INVALID, 2, 1, heads=0)
    refused(INVALID, 2, 1, heads=-6)
    refused(INVALID, 2, 2, n_rows=2, row0=1)   # positions outside the buffer
    for heads in (1, 3, 4, 7, 12):
        refused(FORMAT, 2, 1, heads=heads)
    report(f"B7 bf16={bf16}", R.b1_instantiation(eng, 2, 2, bf16))


# ---------------------------------------------------------------------------------- C. the kProCombine prologue ---
@FORMS
@pytest.mark.parametrize("H", [2, 6, 8])
def test_c1_shapes(eng, H, bf16):
    """chunks in {1, 2, 4, 8} x M in {1, 31, 32, 33, 64, 97, 128}: both row-group forms of every chunk count, a real
    weight, bias and the residual in place; guard rows behind M untouched"""
    report(f"C1 H={H} bf16={bf16}", R.c1_shapes(eng, H, bf16))


@FORMS
@pytest.mark.parametrize("H", [2, 6, 8])
def test_c1_last_tile_of_one_row_is_repeatable(eng, H, bf16):
    """M = 33 and 97, whose last row tile holds one row, repeated behind polluted allocations: the same bits every time"""
    report(f"C1 one-row tile H={H} bf16={bf16}", R.c1_last_tile_of_one_row(eng, H, bf16))


@FORMS
@pytest.mark.parametrize("chunks", [4, 8])
def test_c2_extremes(eng, chunks, bf16):
    report(f"C2 chunks={chunks} bf16={bf16}", R.c2_extremes(eng, chunks, bf16))


@FORMS
def test_c3_kernel_to_prologue(eng, bf16):
    R.c3_kernel_to_prologue(eng, bf16)
