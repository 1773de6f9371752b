"""GPU (-m gpu): the four encoder self-attention kernels, one by one, through wt_dbg_encoder_attention_at
(include/wt_debug.h), which calls the launchers with a given shape, given operand scales and rows behind the last clip:

  f32-v0    encoder_attention_f32            (k_attention.hip; a layer's fall-back when its load-time slack check fails)
  split-v1  encoder_attention_split<4, 3>    (k_attention.hip; the same, three bf16 planes)
  planes    encoder_attention_planes<false>  (k_attention_planes.hip; the default, two fp16 planes)
  bf16      encoder_attention_planes<true>   (the bf16 storage mode)

tests/test_gpu_kernels.py holds them to float64 at T in {64, 100, 128, 300, 333, 400, 1500} with scales taken from
standard-normal data.  This file adds what that leaves open (inputs, reference and bars: tests/attn_cases.py, which
tests/test_encoder_attention_reference.py holds to a plain float32 attention on the CPU):

  a  lengths below, at and one past the 64-key tile and the 128-query block, T = 1, and a grid of every residue mod 8
     (every kernel permutes blockIdx with a formula in gridDim.x & 7);
  b  the plane kernel at the scales the ENGINE passes: f16_scale_for of load-time bounds up to kF16Slack = 2^12 above the
     data, where the low planes reach fp16's subnormals, and V far from unit magnitude;
  c  isolation: (clip, head) reads its own 64 columns of its own T rows only, bit for bit, and one clip alone gives the
     same bits;
  d  softmax edges: a dominating key at tile edges and in a nearly empty last tile, one key with all others underflowing,
     equal scores, falling scores;
  e  refusals before anything is launched;
  f  the two plane kernels (MFMA operands written in registers just before the MFMA: DESIGN section 25) six times behind
     polluted allocations: the same bits every call.

Every launch of a, b and d has three guard rows of NaN behind the last clip and an output pre-filled with a NaN bit
pattern: no sentinel may remain in a clip's rows, and the output's guard rows must come back bit for bit.

The reference is the float64 softmax(q k^T / 8) v per (clip, head), for bf16 on the bf16-rounded input.  Tolerances
(none is new, attn_cases.tolerances): 2e-5 max(1, max|v|) for the three fp32-grade forms, 2^-8 max|ref| + 4e-3 max(1,
max|v|) for bf16, per (clip, head)."""
import numpy as np
import pytest

import attn_cases as ac

pytestmark = pytest.mark.gpu

GUARD = 3
FORM_IDS = list(ac.FORMS)
SENTINEL = {0: (np.uint32, 0x7FC5A5A5), 1: (np.uint16, 0x7EAD), 2: (np.uint16, 0x7FAD)}  # NaN bits of fp32, fp16, bf16


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def sentinel_out(kind, rows, d):
    utype, bits = SENTINEL[kind]
    out = np.full(((2, rows, d) if kind == 1 else (rows, d)), bits, utype)
    return out.view({0: np.float32, 1: np.float16, 2: np.uint16}[kind])


def with_guard(qkv, guard=GUARD):
    return np.concatenate([np.asarray(qkv, np.float32), np.full((guard, qkv.shape[1]), np.nan, np.float32)])


def run(eng, form, qkv, B, T, H, scales=None, guard=GUARD):
    """One launch over qkv [B * T][3 * 64 * H] + `guard` NaN rows into a sentinel-filled output.  Returns (values [B * T]
    [64 * H] float32, raw bits of those rows); asserts that the launch wrote every cell of the clips' rows and none of the
    guard rows."""
    kind, variant = ac.FORMS[form]
    if kind == 1 and scales is None:
        scales = ac.plane_scales(qkv, B, T, H)
    out = sentinel_out(kind, B * T + guard, 64 * H)
    raw, values = eng.dbg_encoder_attention_at(kind, with_guard(qkv, guard), B, T, H, out, variant=variant, scales=scales)
    utype, bits = SENTINEL[kind]
    raw = raw.view(utype).reshape(-1, B * T + guard, 64 * H)
    assert not (raw[:, :B * T] == bits).any(), "a cell of a clip's rows was not written"
    assert (raw[:, B * T:] == bits).all(), "rows behind the last clip were written"
    return values[:B * T], raw[:, :B * T]


# ------------------------------------------------------------------------------------------- a: lengths and grids ---

@pytest.mark.parametrize("form", FORM_IDS)
@pytest.mark.parametrize("B,T,H,grid", ac.SWEEP)
def test_length_and_grid_sweep(eng, form, B, T, H, grid):
    assert B * H * ((T + 127) // 128) == grid
    qkv, refs = ac.normal_case(B, T, H)
    got, _ = run(eng, form, qkv, B, T, H)
    x, ref = refs[form == "bf16"]
    ac.check_against(form, got, ref, x, B, T, H, f"a ({B}, {T}, {H})")


# ------------------------------------------------------------------------------- b: the scales the engine passes ---

@pytest.mark.parametrize("case", list(ac.SCALE_CASES))
@pytest.mark.parametrize("B,T,H", ac.SCALE_SHAPES)
def test_planes_at_engine_scales(eng, B, T, H, case):
    """launch_encoder_attention_planes with q, k, v scales = f16_scale_for(2^j x the data maximum), out scale = v scale.
    A plane pair holds x to max(2^-22 |x|, 2^-39 bound): at j = 12 about 2^-27 of the maximum per element, far inside the
    bar, which is the same for every j.
    Measured on the MI355X, largest error over both shapes: j = 0 and 6: 3.85e-7, j = 12: 4.29e-7, (12, 0, 6): 3.85e-7,
    V x 2^8: 9.84e-5 (bar 2e-5 max|v|, about 2e-2), V x 2^-10: 3.8e-10; at most 0.006 of the bar."""
    j, log2_v = ac.SCALE_CASES[case]
    qkv, ref = ac.scale_case(B, T, H, log2_v)
    scales = ac.plane_scales(qkv, B, T, H, j)
    assert scales[3] == scales[2]
    got, _ = run(eng, "planes", qkv, B, T, H, scales=scales)
    ac.check_against("planes", got, ref, qkv, B, T, H, f"b {case} ({B}, {T}, {H}) scales={scales.tolist()}")


# -------------------------------------------------------------------------------------------------- c: isolation ---

@pytest.mark.parametrize("form", FORM_IDS)
@pytest.mark.parametrize("B,T,H", ac.ISOLATION_SHAPES)
def test_clip_and_head_isolation(eng, form, B, T, H):
    """Each block's arithmetic depends on its own (clip, head, query block) only: with every element outside (b*, h*)
    replaced by NaN (other clips, the other heads' q, k and v columns, the guard rows) the 64 columns x T rows of (b*, h*)
    are bit-identical to the clean run, and so is clip b* run alone as a B = 1 call.  All kernels clamp rows past T to
    row T - 1 and multiply by a zero probability: a read of row T (the next clip, or the guard) would turn 0 * NaN into
    NaN here, where finite data hides it."""
    qkv = ac.normal_case(B, T, H)[0]
    d = 64 * H
    scales = ac.plane_scales(qkv, B, T, H)
    clean, clean_bits = run(eng, form, qkv, B, T, H, scales=scales)
    assert np.isfinite(clean).all()
    for bs, hs in ((0, 0), (B - 1, H - 1)):
        rows, cols = slice(bs * T, (bs + 1) * T), slice(hs * 64, (hs + 1) * 64)
        x = np.full_like(qkv, np.nan)
        for third in range(3):
            c = slice(third * d + hs * 64, third * d + (hs + 1) * 64)
            x[rows, c] = qkv[rows, c]
        kind, variant = ac.FORMS[form]
        out = sentinel_out(kind, B * T + GUARD, d)
        raw, values = eng.dbg_encoder_attention_at(kind, with_guard(x), B, T, H, out, variant=variant, scales=scales)
        bits = raw.view(SENTINEL[kind][0]).reshape(-1, B * T + GUARD, d)
        assert np.isfinite(values[rows, cols]).all(), (bs, hs)
        assert np.array_equal(bits[:, rows, cols], clean_bits[:, rows, cols]), (bs, hs)
        assert (bits[:, B * T:] == SENTINEL[kind][1]).all(), (bs, hs)
        alone, alone_bits = run(eng, form, qkv[rows], 1, T, H, scales=scales)
        assert np.array_equal(alone_bits, clean_bits[:, rows]), bs


# ---------------------------------------------------------------------------------------------- d: softmax edges ---

@pytest.mark.parametrize("form", FORM_IDS)
@pytest.mark.parametrize("case", ac.EDGE_CASES)
def test_softmax_edges(eng, form, case):
    T, qkv, expected = ac.edge_case(case)
    got, _ = run(eng, form, qkv, 1, T, 1)
    ac.check(form, got, qkv, 1, T, 1, f"d {case}")
    want = ac.edge_expected(form, T, qkv, expected)
    if want is not None:  # the closed form: v[0], or the column mean of V
        x = ac.reference_input(form, qkv)
        ac.check_against(form, got, np.tile(want, (T, 1)), x, 1, T, 1, f"d {case} closed form")


# -------------------------------------------------------------------------------------------------- e: refusals ---

REFUSALS = {"T=0": dict(T=0), "batch=0": dict(batch=0), "heads=0": dict(heads=0), "guard_rows=-1": dict(guard_rows=-1),
            "variant=2": dict(variant=2), "variant=4": dict(variant=4)}


@pytest.mark.parametrize("form,name", [(f, n) for f in FORM_IDS for n in REFUSALS if f == "f32-v0" or not n.startswith("variant")])
def test_refusals(eng, pkg, form, name):
    """WT_ERR_INVALID_ARG before anything is launched, the output untouched, and a valid launch afterwards still works.
    The valid launch these depart from: (2, 5, 2) with 3 guard rows."""
    kind, variant = ac.FORMS[form]
    B, T, H = 2, 5, 2
    qkv = ac.normal_case(B, T, H)[0]
    a = dict(batch=B, T=T, heads=H, guard_rows=GUARD, variant=variant, scales=ac.plane_scales(qkv, B, T, H))
    a.update(REFUSALS[name])
    out = sentinel_out(kind, B * T + GUARD, 64 * H)
    with pytest.raises(pkg.WtError) as ei:
        eng.dbg_encoder_attention_at(kind, with_guard(qkv), out=out, copy=False, **a)
    assert ei.value.code == 1, name
    assert (out.view(SENTINEL[kind][0]) == SENTINEL[kind][1]).all(), name
    got, _ = run(eng, form, qkv, B, T, H)
    ac.check(form, got, qkv, B, T, H, f"e after {name}")


# ------------------------------------------------------------------------------------ f: the same bits every call ---

# one key; one key past a 32-key PV step, past the 64-key tile and past the 128-query block (all of them in ac.SWEEP)
REPEAT_SHAPES = [(1, 1, 1), (3, 33, 3), (11, 65, 1), (1, 129, 7)]
HUGE = np.float32([3e34, -7e33, 1e30, 5e36, -2e34, 1e25])


@pytest.mark.parametrize("form", ["planes", "bf16"])
@pytest.mark.parametrize("B,T,H", REPEAT_SHAPES)
def test_same_bits_every_call(eng, form, B, T, H):
    """Six calls, each behind a call of the same shape on the input times a huge number, so that the allocations the
    launch reuses (and whatever registers and LDS the polluting launch left) held huge values, infinities or NaN: every
    call inside the form's bar and bit-identical to the first.  A probability plane that an MFMA reads before its
    conversion has landed (tools/isa_hazards.py holds the distance in the ISA; this is the run-time side) is a timing
    defect and shows as a difference between calls, as pack_bf16x2's did in the decoder."""
    kind, variant = ac.FORMS[form]
    qkv, refs = ac.normal_case(B, T, H)
    x, ref = refs[form == "bf16"]
    scales = ac.plane_scales(qkv, B, T, H)
    first = None
    for rep in range(6):
        eng.dbg_encoder_attention_at(kind, with_guard(qkv * HUGE[rep]), B, T, H, sentinel_out(kind, B * T + GUARD, 64 * H),
                                     variant=variant, scales=scales)
        got, bits = run(eng, form, qkv, B, T, H, scales=scales)
        ac.check_against(form, got, ref, x, B, T, H, f"f ({B}, {T}, {H}) call {rep}")
        first = bits if first is None else first
        assert np.array_equal(bits, first), f"f ({B}, {T}, {H}): call {rep} differs from call 0 in {int((bits != first).sum())} cells"
