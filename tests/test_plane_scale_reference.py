"""CPU: the cases, bars and models of tests/test_gpu_plane_scales.py (tests/plane_scale_ref.py) held to
what they claim, without a GPU.

  * the numpy emulation of the plane GEMM — three exact products on the fp16 planes — meets A QUARTER of every bar of G1,
    G2 and G3: a bar an honest implementation of the same arithmetic could not meet would say nothing about the kernel;
  * three one-defect emulations (a subnormal lo read as zero; out_scale[0] for every segment; a split that saturates where
    the format gives inf) each FAIL their case at the full bar: the bars see what they are there to see;
  * f16_scale_for, the Python copy and the library's own, against kernels.h's contract in exact arithmetic;
  * 4.1's claim 1, sound bounds: no intermediate of the float64 encoder graph exceeds the model's per-channel bound, or
    16384 once multiplied by the model's scale, for any of the mel inputs inside kMelBound — no exception allowed;
  * the verdicts the float64 model gives on the four micro weight variants."""
import functools

import numpy as np
import pytest

import attn_cases as ac
import plane_scale_ref as ps
from fp64_encoder import encoder_fp64

QUARTER = 0.25


# ----------------------------------------------------------------------------------------------- f16_scale_for ---

def test_f16_scale_for_python_and_library_meet_the_contract(pkg):
    """every power of two 2^-140 .. 2^127 with its float32 neighbours, 0, -1, NaN, inf: the bounds below 16384 / FLT_MAX
    and +inf are where the quotient form returned 0.5"""
    for b in ps.scale_sweep_bounds():
        want = ps.f16_scale_exact(b)
        assert ac.f16_scale_for(b) == want, b
        assert pkg.f16_scale_for(b) == want, b
    assert ps.f16_scale_exact(1e-36) == 2.0 ** 24 and ps.f16_scale_exact(float("inf")) == 2.0 ** -24
    assert ps.f16_scale_exact(16384.0) == 1.0 and ps.f16_scale_exact(np.nextafter(np.float32(16384), np.float32(1e9))) == 0.5


def test_tile_table_is_the_launchers_plan(pkg):
    """the n_cu -> tile table of the cases against plane_gemm_plan itself (no GPU work): a changed cost model fails here and
    in the GPU test, it does not silently drop a tile"""
    for (M, N, K) in ps.G1_SHAPES:
        for n_cu, tile in ps.TILES[(M, N)].items():
            for epi, planes in ((1, False), (5, False), (1, True), (3, True)):
                assert pkg.plane_gemm_plan(M, N, K, epi, planes, False, n_cu).tile == tile, (M, N, K, epi, planes, n_cu)
    assert sorted(ps.TILES[(193, 384)].values()) == [0, 1, 2]


# --------------------------------------------------------------------------------------- emulation against bars ---

@pytest.mark.parametrize("shape", ps.G1_SHAPES)
def test_emulation_meets_a_quarter_of_the_g1_bars(shape):
    for epi in (1, 5):
        for j in ps.J_INSIDE + ps.J_OUTSIDE:
            r = ps.run_f32(ps.emulate, shape, j, epi, frac=QUARTER)
            print(f"G1 {shape} epi {epi} j {j}: emulation at {r:.3f} of the bar")


def test_emulation_meets_a_quarter_of_the_g2_bars():
    for j in (0, 12):
        r = ps.run_f32(ps.emulate, ps.G_SHAPE, j, 1, wide=True, frac=QUARTER)
        print(f"G2 j {j}: emulation at {r:.3f} of the bar")


def test_wide_operands_are_beyond_the_max_norm_bar_at_the_slack_edge():
    """why G2 has an element-wise bar and kF16Slack exists: at j = 12 the float64-EXACT product of the split operands is
    itself above the 2e-6 max|ref| bar of G1 on these operands"""
    M, N, K = ps.G_SHAPE
    A, W, bias, _, prod = ps.operands(M, N, K, True)
    sa, sw = ps.scale_at(A, 12), ps.scale_at(W, 0)
    (ah, al), (wh, wl) = ps.split(A, sa), ps.split(W, sw)
    a = (ah.astype(np.float64) + al.astype(np.float64)) / sa
    w = (wh.astype(np.float64) + wl.astype(np.float64)) / sw
    err = np.abs(a @ w.T + bias - prod).max() / np.abs(prod).max()
    print(f"exact product of the split operands at j = 12: {err:.2e} of max|ref|")
    assert err > 2e-6


@pytest.mark.parametrize("form", list(ps.G3_FORMS))
def test_emulation_meets_a_quarter_of_the_g3_bars(form):
    for epi in (1, 3):
        r, ties = ps.run_planes(ps.emulate, form, epi, frac=QUARTER)
        print(f"G3 {form} epi {epi}: emulation at {r:.3f} of the bar, {ties} ties")


def test_emulation_passes_g4():
    ps.run_g4_operand(ps.emulate)
    ps.run_g4_output(ps.emulate)
    ps.run_g4_convert(ps.convert_emulation)


# ----------------------------------------------------------------------------------------------------- mutants ---

def test_mutant_that_flushes_subnormal_lo_fails_g1_and_g2_at_the_full_bar():
    flush = functools.partial(ps.emulate, mutant="flush")
    for shape, j, wide in ((ps.G_SHAPE, 12, False), (ps.G_SHAPE, 15, False), (ps.G_SHAPE, 18, False), (ps.G_SHAPE, 12, True)):
        with pytest.raises(AssertionError, match="of the bar") as ei:
            ps.run_f32(flush, shape, j, 1, wide=wide)
        print(ei.value)
    ps.run_f32(flush, ps.G_SHAPE, 0, 1)  # at the tightest scale no lo of a typical element is subnormal: nothing to see


def test_mutant_with_one_out_scale_fails_g3():
    with pytest.raises(AssertionError, match="of the bar"):
        ps.run_planes(functools.partial(ps.emulate, mutant="scale0"), "qkv-12-0-6", 1)
    ps.run_planes(functools.partial(ps.emulate, mutant="scale0"), "one-j6", 1)  # one segment: the defect is out of reach


def test_mutant_that_saturates_fails_g4():
    sat = functools.partial(ps.emulate, mutant="saturate")
    with pytest.raises(AssertionError, match="saturated"):
        ps.run_g4_operand(sat)
    with pytest.raises(AssertionError, match="0x7bff"):
        ps.run_g4_output(sat)
    with pytest.raises(AssertionError, match="0xfbff"):
        ps.run_g4_convert(functools.partial(ps.convert_emulation, mutant="saturate"))


# ------------------------------------------------------------------------------------------ derivation (G5) ---

@pytest.fixture(scope="module")
def variants(assets, tmp_path_factory):
    """name -> (dims, tensors, model) of the four micro weight variants"""
    from wtw import read_wtw
    src, _ = assets("micro")
    d = tmp_path_factory.mktemp("plane-scale-variants")
    out = {}
    for name in ps.WEIGHT_VARIANTS:
        p = str(d / (name + ".wtw"))
        ps.write_variant(name, src + ".wtw", p)
        dims, t = read_wtw(p)
        out[name] = (dims, t, ps.encoder_bounds(dims, t))
    return out


@pytest.mark.parametrize("name", ps.WEIGHT_VARIANTS)
def test_bounds_are_sound_on_the_float64_graph(variants, name):
    """Claim 1 of DESIGN 4.1.  A triangle-inequality bound holds with no exception: every element of every operand, for
    every mel, is inside its channel's bound and, times the scale its planes take, inside 16384."""
    dims, t, model = variants[name]
    assert (dims["n_audio_state"], dims["n_audio_layer"], dims["n_audio_ctx"]) == (128, 2, 100)
    assert len(model.records) == 13
    for what, mel in ps.sound_mels(dims, t).items():
        assert np.abs(mel).max() <= ps.MEL_BOUND
        taps = {}
        encoder_fp64(dims, t, mel, taps)
        taps["mel"] = mel.T
        assert set(taps) == set(model.ops)
        closest = 0.0
        for key, x in taps.items():
            x = np.abs(x) * (float(ac.KQ) if key.startswith("q.") else 1.0)
            op = model.ops[key]
            over = x.max(axis=0) / np.broadcast_to(op.bound, x.shape[1:])
            assert over.max() <= 1.0 + 1e-12, f"{name}, {what}: {key} channel {int(over.argmax())} at {over.max():.6f} of its bound"
            assert x.max() * model.scales[key] <= 16384.0 * (1.0 + 1e-12), (name, what, key)
            closest = max(closest, float(over.max()))
        print(f"{name}, {what}: the closest operand element is at {closest:.3f} of its bound")


def test_verdicts_of_the_float64_model(variants):
    """The contractions the model sends off the plane kernels (plane_scale_ref.EXPECTED_FALLBACKS).  On tiny one value
    channel 10^4 x larger flags layer 0's attention and its out-projection (4.1); on micro it cannot — a row outlier is
    worth at most sqrt(d) = 3.5 bits at d = 128 and leaves 1.84 bits of slack — and the model flags nothing there.  The
    value-BIAS outlier flags exactly those two; the other variants flag none."""
    for name in ps.WEIGHT_VARIANTS:
        model = variants[name][2]
        flagged = [int(i) for i in np.flatnonzero(~model.ok)]
        print(f"{name}: flagged {flagged}, min slack {model.min_slack_bits:.3f} bits")
        assert flagged == ps.EXPECTED_FALLBACKS[name], name
        assert model.fallbacks == len(flagged)
        # no scale or verdict of the model sits within 2^-18 of a boundary: the GPU test's exceptions are for the engine's
        # float32 storage alone
        n = len(model.records)
        for i, r in enumerate(model.records):
            pairs = [(r[4], r[5]), (r[6], r[7]), (r[8], r[9])] if ps.is_attention(i, n) else [(r[3], r[4])]
            for bound, typ in pairs:
                assert i == 0 or not ps.near_boundary(bound), (name, i)  # (conv1's is the constant kMelBound = 8, exact)
                assert abs(bound / (ps.SLACK * typ) - 1.0) > 2.0 ** -18, (name, i)
