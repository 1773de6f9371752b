"""GPU (-m gpu): the plane GEMM at LOAD-TIME scales, and the derivation of those scales.

The other plane GEMM taps take a_scale and w_scale from the uploaded data's own maximum — the tightest scale there is,
and one the engine never has: its a_scale comes from a weight-derived bound 2^4 .. 2^12 above the data.  Here every
scale is the caller's (wt_dbg_gemm_planes_scaled), and the engine's own derivation is read back
(wt_dbg_encoder_scales) and held to a float64 restatement of DESIGN 4.1.  Cases, references, bars and the bounds model
are tests/plane_scale_ref.py; tests/test_plane_scale_reference.py holds them to a numpy emulation without a GPU.

  G1  the ladder: a_scale = f16_scale_for(2^j max|A|), j = 0, 6, 12 inside kF16Slack and 15, 18 outside, three shapes,
      every tile the cost model reaches at them, bias and bias | residual epilogues
  G2  wide operands: A's columns down to 2^-10 of its maximum, so that lo planes of typical elements are subnormal
  G3  plane output with three segment scales (12, 0, 6) and with one; hi the fp16 nearest to hi + lo; guard rows
  G4  out of range: an operand element, an output column, a converted cell past fp16's range are inf, not saturated, and
      touch nothing else; f16_scale_for over the whole float32 exponent range
  G5  the derivation on five micro weight files, record by record, and the launches that follow from it

Every case first asserts what the launcher's plan function says it will launch."""
import numpy as np
import pytest

import plane_scale_ref as ps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def tiles(pkg, shape, epi, planes_out=False):
    """[(n_cu, tile name)] of the shape, after asserting the launcher's plan for each"""
    M, N, K = shape
    out = []
    for n_cu, tile in ps.TILES[(M, N)].items():
        plan = pkg.plane_gemm_plan(M, N, K, epi, planes_out, False, n_cu)
        assert plan.tile == tile and not plan.fused, (shape, epi, n_cu, plan.kernel)
        out.append((n_cu, plan.kernel))
    return out


# ------------------------------------------------------------------------------------------------------- G1, G2 ---

@pytest.mark.parametrize("epi", [1, 5])
@pytest.mark.parametrize("shape", ps.G1_SHAPES)
def test_g1_ladder_of_engine_scales(pkg, eng, shape, epi):
    """Inside the slack (j <= 12) the sibling tests' own bars hold with nothing added: 2e-6 max|ref|, 3e-6 with the
    residual.  Outside it the error may grow as the fp16 format says and no faster: 2 x the product model, per element."""
    for n_cu, kernel in tiles(pkg, shape, epi):
        for j in ps.J_INSIDE + ps.J_OUTSIDE:
            r = ps.run_f32(eng.dbg_gemm_planes_scaled, shape, j, epi, n_cu=n_cu)
            print(f"[plane-scale] G1 {shape} epi {epi} j {j:2d} {kernel}: worst error / bar {r:.3f}")


def test_g2_wide_operands_with_subnormal_lo_planes(pkg, eng):
    for n_cu, kernel in tiles(pkg, ps.G_SHAPE, 1):
        for j in (0, 12):
            r = ps.run_f32(eng.dbg_gemm_planes_scaled, ps.G_SHAPE, j, 1, n_cu=n_cu, wide=True)
            print(f"[plane-scale] G2 {ps.G_SHAPE} epi 1 j {j:2d} {kernel}: worst error / bar {r:.3f}")


# ----------------------------------------------------------------------------------------------------------- G3 ---

@pytest.mark.parametrize("epi", [1, 3])
@pytest.mark.parametrize("form", list(ps.G3_FORMS))
def test_g3_plane_output_at_segment_scales(pkg, eng, form, epi):
    for n_cu, kernel in tiles(pkg, ps.G_SHAPE, epi, True):
        r, ties = ps.run_planes(eng.dbg_gemm_planes_scaled, form, epi, n_cu=n_cu)
        print(f"[plane-scale] G3 {form} epi {epi} {kernel}: worst error / bar {r:.3f}, {ties} of {ps.G_SHAPE[0] * ps.G_SHAPE[1]} "
              "hi + lo on a tie")


# ----------------------------------------------------------------------------------------------------------- G4 ---

def test_g4_operand_past_the_range_is_inf_in_its_row_only(pkg, eng):
    for n_cu, _ in tiles(pkg, ps.G_SHAPE, 1):
        ps.run_g4_operand(eng.dbg_gemm_planes_scaled, n_cu=n_cu)


def test_g4_output_past_the_range_is_inf_not_saturated(pkg, eng):
    for n_cu, _ in tiles(pkg, ps.G_SHAPE, 1, True):
        ps.run_g4_output(eng.dbg_gemm_planes_scaled, n_cu=n_cu)


def test_g4_converted_cell_past_the_range_is_inf_not_saturated(eng):
    ps.run_g4_convert(eng.dbg_f32_to_planes)


def test_g4_f16_scale_for_over_the_exponent_range(pkg):
    for b in ps.scale_sweep_bounds():
        assert pkg.f16_scale_for(b) == ps.f16_scale_exact(b), b


def test_launcher_refusals_come_back_as_status_codes(pkg, eng):
    M, N, K = ps.G_SHAPE
    A, W, bias, _, _ = ps.operands(M, N, K)
    for kw in (dict(a_scale=0.0, w_scale=1.0), dict(a_scale=1.0, w_scale=float("nan")),
               dict(a_scale=1.0, w_scale=1.0, seg=100, planes=True), dict(a_scale=1.0, w_scale=1.0, seg=64, planes=True),
               dict(a_scale=1.0, w_scale=1.0, epi=9), dict(a_scale=1.0, w_scale=1.0, epi=5, planes=True)):
        planes = kw.pop("planes", False)
        given = ps.fill16(M, N) if planes else ps.fill32(M, N)
        with pytest.raises(pkg.WtError) as ei:
            eng.dbg_gemm_planes_scaled(A, W, bias, given, **kw)
        assert ei.value.code == 1, kw


# ----------------------------------------------------------------------------------------------------------- G5 ---

CAP = 2  # boundary exceptions allowed per variant


@pytest.fixture(scope="module")
def variant_files(assets, tmp_path_factory):
    src, vocab = assets("micro")
    d = tmp_path_factory.mktemp("plane-scale-variants")
    made = {}

    def get(name):
        if name not in made:
            made[name] = str(d / name)
            ps.write_variant(name, src + ".wtw", made[name] + ".wtw")
        return made[name], vocab

    return get


@pytest.mark.parametrize("name", ps.WEIGHT_VARIANTS)
def test_g5_engine_derivation_matches_the_float64_model(pkg, variant_files, name):
    """Every record of wt_dbg_encoder_scales against encoder_bounds: scales and verdicts equal — except where the model's
    bound lies within 2^-18 of a power-of-two boundary of 16384 / bound, or of the slack threshold, where the engine's
    float32 storage may land on the other side (counted, at most CAP) — bound and typical magnitude to 1e-5, and the
    engine's three counters."""
    from wtw import read_wtw
    prefix, vocab = variant_files(name)
    dims, t = read_wtw(prefix + ".wtw")
    model = ps.encoder_bounds(dims, t)
    e = pkg.Engine(prefix, vocab, True)
    rec = e.dbg_encoder_scales().astype(np.float64)
    counters = [e.get_option(k) for k in ("f16_fallbacks", "f16_contractions", "f16_min_slack_millibits")]
    e.set_option("force_fallback", 1)  # the records are the load-time verdicts, whatever is forced
    assert np.array_equal(e.dbg_encoder_scales().astype(np.float64), rec)
    e.close()
    n = len(model.records)
    assert rec.shape == (n, 10) and n == 13
    exceptions = 0
    for i in range(n):
        got, want = rec[i], model.records[i]
        if ps.is_attention(i, n):
            scales, ok, ops = (0, 1, 2), 3, ((4, 5), (6, 7), (8, 9))
            a_of = {0: 4, 1: 6, 2: 8}
        else:
            scales, ok, ops = (0,), 2, ((3, 4),)
            a_of = {0: 3}
            assert got[1] == want[1], (name, i, "w_scale")
            assert not got[5:].any()
        for c in scales:
            if got[c] != want[c]:
                assert ps.near_boundary(want[a_of[c]]) and got[c] / want[c] in (0.5, 2.0), (name, i, c, got[c], want[c])
                exceptions += 1
        if bool(got[ok]) != bool(want[ok]):
            assert any(abs(want[b] / (ps.SLACK * want[ty]) - 1.0) < 2.0 ** -18 for b, ty in ops), (name, i, "verdict")
            exceptions += 1
        for b, ty in ops:
            assert abs(got[b] / want[b] - 1.0) < 1e-5 and abs(got[ty] / want[ty] - 1.0) < 1e-5, (name, i, got, want)
    print(f"[plane-scale] G5 {name}: {n} records, {exceptions} boundary exceptions, fall-backs {counters[0]}, "
          f"min slack {counters[2] / 1000.0:.3f} bits (model {model.min_slack_bits:.3f})")
    assert exceptions <= CAP
    cleared = sum(1 for i in range(n) if not rec[i][3 if ps.is_attention(i, n) else 2])
    assert counters[0] == cleared and counters[1] == n
    assert abs(counters[2] - round(1000.0 * model.min_slack_bits)) <= 2
    if exceptions == 0:
        assert [int(i) for i in np.flatnonzero(~model.ok)] == ps.EXPECTED_FALLBACKS[name]


@pytest.mark.parametrize("name", ["v-row-1e4", "v-bias-1e4"])
def test_g5_launches_follow_the_verdicts(pkg, variant_files, name):
    """One synchronous one-clip pass: a gemm_split16_tile launch for every cleared GEMM verdict, an encoder_attention_split
    launch for every cleared attention verdict, plane launches for all the others (11 GEMMs — conv1, conv2, four per
    layer, cross-KV — and 2 attentions on micro).  The row outlier clears nothing on micro, the bias outlier layer 0's
    attention and out-projection: what test_fp16_split_falls_back_per_contraction... sees on tiny."""
    prefix, vocab = variant_files(name)
    e = pkg.Engine(prefix, vocab, True)
    rec = e.dbg_encoder_scales()
    n = len(rec)
    att = [i for i in range(n) if ps.is_attention(i, n)]
    gemm_off = sum(1 for i in range(n) if i not in att and not rec[i][2])
    attn_off = sum(1 for i in att if not rec[i][3])
    assert [gemm_off, attn_off] == ([1, 1] if name == "v-bias-1e4" else [0, 0])
    e.set_option("stop_at_eot", 0)
    e.set_option("max_tokens", 5)
    e.set_prompt([3, 5, 7, 11])
    e.set_option("kernel_timers", 1)
    mel = np.random.default_rng(31).uniform(-1.0, 1.5, size=(1,) + e.mel_shape).astype(np.float32)
    e.encdec_tokens_batch(mel)
    ks = e.kernel_stats()
    e.close()
    launches = lambda k: ks[k]["launches"] if k in ks else 0
    assert launches("gemm_split16_tile") == gemm_off and launches("gemm_planes") == n - len(att) - gemm_off, ks
    assert launches("encoder_attention_split") == attn_off and launches("encoder_attention_planes") == len(att) - attn_off, ks
