"""CPU: the references of tests/decoder_attn_ref.py against themselves.
(a) The float64 per-chunk statistics merge to unchunked attention for every chunk geometry the GPU test runs, empty chunks
    included.
(b) A plain float32 emulation of each kernel (Emu: fp32 dot products, fp32 exp, the kernels' chunk and merge structure) stays
    within ONE QUARTER of every bar of every case of sections A, B and C: the evidence that a correct fp32 kernel can meet
    them.  The cases are the functions the GPU test runs, with Emu in the Engine's place.
(c) Emulations with one subtle defect each (a past key of the last load round counted once, a stale cache row used, rows
    written at b * npos + p, a neighbouring head's records combined, an empty chunk given weight) fail the case built
    for that defect at the FULL bars: the cases can tell."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decoder_attn_ref as R  # noqa: E402

FORMS = pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
QUARTER = 0.25


@pytest.fixture(scope="module")
def emu():
    return R.Emu()


# ---------------------------------------------------------------------------------------------------------- (a) ---
@pytest.mark.parametrize("T,chunks", R.GEOMETRY + [(1500, 8)])
def test_chunked_merge_equals_unchunked_attention(T, chunks):
    rng = np.random.default_rng(T * 10 + chunks)
    B, H = 2, 2
    s = rng.standard_normal((3, B, H, T)) * 3
    V = rng.standard_normal((1, B, H, T, 64))
    mx, lse, mean, empty = R.chunk_stats(s, V, T, chunks)
    bounds = R.chunk_bounds(T, chunks)
    assert [hi <= lo for lo, hi in bounds] == list(empty)
    assert sum(max(0, hi - lo) for lo, hi in bounds) == T and all(lo == c * bounds[0][1] for c, (lo, _) in enumerate(bounds))
    assert empty.sum() == {(9, 4): 1, (9, 8): 3, (15, 4): 0, (15, 8): 0, (17, 8): 2, (33, 8): 1, (65, 8): 0}.get((T, chunks), 0)
    assert np.isneginf(lse[..., empty]).all() and np.isfinite(lse[..., ~empty]).all() and (mx[..., ~empty] <= lse[..., ~empty]).all()
    ref = R.attention_ref(s, V)
    assert np.abs(R.merge_chunks(lse, mean) - ref).max() < 1e-13
    # the same through records as the kernel lays them out (o unnormalised, m, l) and the prologue's combine
    rec = np.zeros((3 * B, H, chunks, 68))
    l = np.where(empty, 0.0, np.exp(lse - mx))
    rec[..., :64] = (mean * l[..., None]).reshape(3 * B, H, chunks, 64)
    rec[..., 64] = np.where(empty, float(R.EMPTY_M), mx).reshape(3 * B, H, chunks)
    rec[..., 65] = l.reshape(3 * B, H, chunks)
    assert np.abs(R.combine_ref(rec).reshape(3, B, H, 64) - ref).max() < 1e-13


def test_bars_come_from_the_inputs():
    """ds is 65 * 2^-24 * max_j sum_c |q_c k_jc| / 8, for the self-attention rows and for the cross-attention chunks"""
    rng = np.random.default_rng(1)
    qkv = rng.standard_normal((2, 3 * 128)).astype(np.float32)
    kc, vc = np.zeros((2, 32, 128), np.float32), np.zeros((2, 32, 128), np.float32)
    kc[:, :3], vc[:, :3] = rng.standard_normal((2, 3, 128)), rng.standard_normal((2, 3, 128))
    _, kc2, vc2, ds, vmax = R.self_ref(qkv, kc, vc, 3, 1, False)
    q, K = qkv[1, 64:128].astype(np.float64), kc2[1, :4, 64:128].astype(np.float64)
    assert np.isclose(ds[1, 1], 65 * 2.0 ** -24 * (np.abs(K) * np.abs(q)).sum(1).max() / 8, rtol=1e-12)
    assert vmax[1, 1] == np.abs(vc2[1, :4, 64:128]).max()
    inp = R.cross_inputs(rng, 2, 2, 9, 1, False)
    ref = R.cross_ref(*inp, 8, 1, False)
    q = R.query_ref(*inp[:5])[1, :64]
    want = 65 * 2.0 ** -24 * (np.abs(inp[5][1, 0, 2:4].astype(np.float64)) * np.abs(q)).sum(1).max() / 8
    assert np.isclose(ref["ds"][0, 1, 0, 1], want, rtol=1e-12) and list(ref["empty"]) == [False] * 5 + [True] * 3


# ---------------------------------------------------------------------------------------------------------- (b) ---
@FORMS
@pytest.mark.parametrize("H", [2, 6, 8])
def test_emulation_a1_every_position(emu, H, bf16):
    assert R.a1_every_position(emu, H, bf16, QUARTER) <= QUARTER


@FORMS
@pytest.mark.parametrize("pos0,npos,B,H", R.A2_GROUPS)
def test_emulation_a2_prompt_groups(emu, pos0, npos, B, H, bf16):
    assert R.a2_prompt_group(emu, pos0, npos, B, H, bf16, QUARTER) <= QUARTER


@FORMS
@pytest.mark.parametrize("B,pos0,npos", R.A3_WIDTHS)
def test_emulation_a3_chain_widths(emu, B, pos0, npos, bf16):
    assert R.a3_chain_width(emu, B, pos0, npos, bf16, QUARTER) <= QUARTER


@FORMS
@pytest.mark.parametrize("cap", R.A4_CAPS)
def test_emulation_a4_stride_and_stale_rows(emu, cap, bf16):
    assert R.a4_stride_and_stale_rows(emu, cap, bf16, QUARTER) <= QUARTER


@FORMS
def test_emulation_a5_bit_identity(emu, bf16):
    assert R.a5_bit_identity(emu, bf16, QUARTER) <= QUARTER


@FORMS
@pytest.mark.parametrize("regime", R.A6_REGIMES)
def test_emulation_a6_softmax_regimes(emu, regime, bf16):
    assert R.a6_softmax_regime(emu, regime, bf16, QUARTER) <= QUARTER


@FORMS
@pytest.mark.parametrize("H", [2, 6, 8])
@pytest.mark.parametrize("nq", [1, 2, 3, 4])
def test_emulation_b1_instantiations(emu, nq, H, bf16):
    assert R.b1_instantiation(emu, nq, H, bf16, QUARTER) <= QUARTER


@FORMS
def test_emulation_b2_geometry(emu, bf16):
    assert R.b2_geometry(emu, bf16, QUARTER) <= QUARTER
    assert R.b2_full_length(emu, bf16, QUARTER) <= QUARTER


@FORMS
def test_emulation_b3_masked_past_keys(emu, bf16):
    assert R.b3_masked_past_keys(emu, bf16, QUARTER) <= QUARTER


@FORMS
def test_emulation_b4_layernorm_inside(emu, bf16):
    assert R.b4_layernorm_inside(emu, bf16, QUARTER) <= QUARTER


@FORMS
@pytest.mark.parametrize("regime,T,at", R.B5_CASES)
def test_emulation_b5_softmax_regimes(emu, regime, T, at, bf16):
    assert R.b5_softmax_regime(emu, regime, T, at, bf16, QUARTER) <= QUARTER


@FORMS
def test_emulation_b6_bit_identity_and_grouping(emu, bf16):
    worst, _ = R.b6_bit_identity_and_grouping(emu, bf16, QUARTER)
    assert worst <= QUARTER


@FORMS
@pytest.mark.parametrize("H", [2, 6, 8])
def test_emulation_c1_shapes(emu, H, bf16):
    assert R.c1_shapes(emu, H, bf16, QUARTER) <= QUARTER


@FORMS
@pytest.mark.parametrize("H", [2, 6, 8])
def test_emulation_c1_last_tile_of_one_row(emu, H, bf16):
    assert R.c1_last_tile_of_one_row(emu, H, bf16, QUARTER) <= QUARTER


@FORMS
@pytest.mark.parametrize("chunks", [4, 8])
def test_emulation_c2_extremes(emu, chunks, bf16):
    assert R.c2_extremes(emu, chunks, bf16, QUARTER) <= QUARTER


@FORMS
def test_emulation_c3_kernel_to_prologue(emu, bf16):
    R.c3_kernel_to_prologue(emu, bf16)


# ---------------------------------------------------------------------------------------------------------- (c) ---
class PastKeyCounted(R.Emu):
    """the last key of a chunk whose last round of 16 keys is partial enters the sums once more"""

    def dbg_cross_attention_records(self, x, ln_g, ln_b, wq, bq, kc, vc, chunks=2, nq=1, bf16=False, **kw):
        ws = super().dbg_cross_attention_records(x, ln_g, ln_b, wq, bq, kc, vc, chunks, nq, bf16, **kw)
        B, H, T, _ = kc.shape
        q = self._queries(x, ln_g, ln_b, wq, bq).reshape(nq, B, H, 64)
        rec = ws.reshape(nq, B, H, chunks, 68)
        for c, (lo, hi) in enumerate(R.chunk_bounds(T, chunks)):
            if hi > lo and (hi - lo) % 16:
                s = np.einsum("pbhc,bhc->pbh", q, R.f32(kc)[:, :, hi - 1])
                p = np.exp2(s - rec[..., c, 64] * np.float32(R.LOG2E))
                rec[..., c, :64] += p[..., None] * R.f32(vc)[None, :, :, hi - 1]
                rec[..., c, 65] += p
        return ws


class StaleRowUsed(R.Emu):
    """at pos0 = 0 the row 0 the kernel loads before it is written takes the place of the new row 0"""

    def dbg_self_attention(self, qkv, kcache, vcache, pos, npos=1, bf16=False):
        out, kc, vc = super().dbg_self_attention(qkv, kcache, vcache, pos, npos, bf16)
        if pos == 0:
            kc2, vc2 = kc.copy(), vc.copy()
            kc2[:, 0], vc2[:, 0] = kcache[:, 0], vcache[:, 0]
            d = kc.shape[2]
            qkv = np.array(qkv, np.float32).reshape(npos, -1, 3 * d)
            qkv[0, :, d:2 * d], qkv[0, :, 2 * d:] = kcache[:, 0], vcache[:, 0]
            out = super().dbg_self_attention(qkv.reshape(-1, 3 * d), kcache, vcache, pos, npos, bf16)[0]
        return out, kc, vc


class RowsTransposed(R.Emu):
    def dbg_self_attention(self, qkv, kcache, vcache, pos, npos=1, bf16=False):
        out, kc, vc = super().dbg_self_attention(qkv, kcache, vcache, pos, npos, bf16)
        B, d = kc.shape[0], kc.shape[2]
        return np.ascontiguousarray(out.reshape(npos, B, d).transpose(1, 0, 2)).reshape(npos * B, d), kc, vc


class NeighbourHeadCombined(R.Emu):
    def dbg_cross_combine(self, records, W, bias, Rres, B, bf16=False, guard=None):
        rec = R.f32(records).copy()
        rec[5] = np.roll(rec[6], 1, axis=0)  # row 5 combines row 6's records, heads shifted
        return super().dbg_cross_combine(rec, W, bias, Rres, B, bf16, guard)


class EmptyChunkWeighted(R.Emu):
    def dbg_cross_attention_records(self, x, ln_g, ln_b, wq, bq, kc, vc, chunks=2, nq=1, bf16=False, **kw):
        ws = super().dbg_cross_attention_records(x, ln_g, ln_b, wq, bq, kc, vc, chunks, nq, bf16, **kw)
        for c, (lo, hi) in enumerate(R.chunk_bounds(kc.shape[2], chunks)):
            if hi <= lo:
                ws[:, :, c, 65] = 1.0  # the "sum" of an empty chunk as exp2(-1e30 - -1e30)
        return ws


@FORMS
def test_defective_emulations_fail_their_cases(bf16):
    with pytest.raises(AssertionError):
        R.b3_masked_past_keys(PastKeyCounted(), bf16)
    with pytest.raises(AssertionError):
        R.a4_stride_and_stale_rows(StaleRowUsed(), 33, bf16)
    with pytest.raises(AssertionError):
        R.a3_chain_width(RowsTransposed(), 32, 13, 4, bf16)
    with pytest.raises(AssertionError):
        R.c2_extremes(NeighbourHeadCombined(), 4, bf16)
    with pytest.raises(AssertionError):
        R.b2_geometry(EmptyChunkWeighted(), bf16)
