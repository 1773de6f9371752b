"""GPU (-m gpu): the int8 dynamic-range decoder blocks (option decoder_int8): the kernel through
dbg_dec_gemm_i8 (quantised rows and outputs bit for bit), the launcher's refusals, the engine through the option."""
import numpy as np
import pytest

import decoder_int8_ref as ref
from logits_int8_ref import boundary_distance, quantize_rows
from test_gpu_decoder_step import argmax_last, eng, ln64, rel_err  # noqa: F401 (eng: the micro engine fixture)
from test_gpu_logits_int8 import model  # noqa: F401 (micro, micro-bf16, tiny: engine, weights, 2 clips, 6 steps)

pytestmark = pytest.mark.gpu
F32 = np.float32
RESID, BIAS, GELU = 0, 1, 2
GUARD = F32(1.0e30)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_y(pkg, Y, qx, sx, W, bias, R, epi, M):
    """Y from the kernel's own qx / sx and the host's qw / sw: bit for bit (GELU: the project's bar for gelu_erf against
    the float64 GELU of the bit-exact pre-activation); the four rows behind M untouched"""
    qw, sw = pkg.quantize_rows_i8(W)
    pre = ref.gemm(qx, sx, qw, sw, bias, R if epi == RESID else None)
    if epi == GELU:
        assert rel_err(Y[:M], ref.gelu64(pre)) < 3e-6
    else:
        assert np.array_equal(bits(Y[:M]), bits(pre))
    assert (Y[M:] == GUARD).all()


def operands(rng, M, K, N):
    W = (rng.standard_normal((N, K)) / 16).astype(F32)
    return W, rng.standard_normal(N).astype(F32), rng.standard_normal((M, N)).astype(F32)


@pytest.mark.parametrize("M,K,N,epi,in_place", [(1, 128, 32, BIAS, False), (9, 128, 96, GELU, False), (32, 384, 384, RESID, True),
                                                (33, 512, 512, RESID, False), (128, 1536, 384, RESID, False),
                                                (64, 2048, 512, RESID, False)])
def test_rows_from_memory(pkg, eng, M, K, N, epi, in_place):
    rng = np.random.default_rng(M * 7919 + K)
    X = (rng.standard_normal((M, K)) * 10.0 ** rng.uniform(-2, 2, (M, 1))).astype(F32)
    W, bias, R = operands(rng, M, K, N)
    Y, _, qx, sx = eng.dbg_dec_gemm_i8(W, bias, X=X, R=R if epi == RESID else None, in_place=in_place, epi=epi)
    q_ref, s_ref = quantize_rows(X)
    assert np.array_equal(qx, q_ref) and np.array_equal(bits(sx), bits(s_ref))
    check_y(pkg, Y, qx, sx, W, bias, R, epi, M)


def check_ln(pkg, e, rows, W, bias, g_, b_, epi, **src):
    """rows [M][K] float32: what the prologue normalises.  sx within 4 ulp of the float64 LayerNorm's scale, qx equal to the
    quantiser's wherever a * inv is farther than 2e-3 from a rounding boundary and within 1 elsewhere (DESIGN section 37's
    bars for the same LayerNorm code), Y bit for bit from the kernel's own qx / sx"""
    M = rows.shape[0]
    Y, xout, qx, sx = e.dbg_dec_gemm_i8(W, bias, ln_g=g_, ln_b=b_, epi=epi, **src)
    ln = ln64(rows, g_, b_)
    q_ref, s_ref = quantize_rows(ln.astype(F32))
    near = boundary_distance(ln) < 2e-3
    assert near.mean() < 0.01  # (a condition on the inputs)
    assert np.abs(sx.view(np.int32).astype(np.int64) - s_ref.view(np.int32)).max() <= 4
    diff = np.abs(qx.astype(np.int32) - q_ref)
    assert diff.max() <= 1 and not diff[~near].any()
    check_y(pkg, Y, qx, sx, W, bias, None, epi, M)
    return xout


@pytest.mark.parametrize("with_xpart", [False, True])
@pytest.mark.parametrize("M,K,N,epi", [(32, 384, 1152, BIAS), (9, 128, 512, GELU), (64, 512, 2048, GELU)])
def test_layernorm_rows(pkg, eng, M, K, N, epi, with_xpart):
    rng = np.random.default_rng(M * 104729 + K + with_xpart)
    xin = (rng.standard_normal((M, K)) * 2 + 0.5).astype(F32)
    xpart = rng.standard_normal((M, K)).astype(F32) if with_xpart else None
    g_, b_ = rng.standard_normal(K).astype(F32), rng.standard_normal(K).astype(F32)
    W, bias, _ = operands(rng, M, K, N)
    rows = xin + xpart if with_xpart else xin
    xout = check_ln(pkg, eng, rows, W, bias, g_, b_, epi, xin=xin, xpart=xpart)
    assert np.array_equal(bits(xout[:M]), bits(rows if with_xpart else np.zeros_like(rows))) and not xout[M].any()


def test_layer0_embedding_rows_ragged(pkg, eng):
    """3 clips x 3 positions from slot 3; clip 1 started at slot 2, clip 2 at slot 5 (its rows clamp to positional row 0),
    and clip 0's last position clamps to the table's last row"""
    rng = np.random.default_rng(11)
    K, N, B, M = 128, 512, 3, 9
    ids = rng.integers(0, 50, (B, 8))
    tok, posn = rng.standard_normal((50, K)).astype(F32), rng.standard_normal((5, K)).astype(F32)
    g_, b_ = rng.standard_normal(K).astype(F32), rng.standard_normal(K).astype(F32)
    W, bias, _ = operands(rng, M, K, N)
    for pos_start in (None, [0, 2, 5]):
        pe = posn if pos_start else np.concatenate([posn, posn])  # (without pos_start every row must exist)
        rows = ref.embedding_rows(ids, 3, M, tok, pe, pos_start)
        xout = check_ln(pkg, eng, rows, W, bias, g_, b_, BIAS, ids=ids, pos=3, tok_emb=tok, pos_emb=pe, pos_start=pos_start, M=M)
        assert np.array_equal(bits(xout[:M]), bits(rows)) and not xout[M].any()


def test_edge_rows(pkg, eng):
    rng = np.random.default_rng(5)
    K, N, M = 128, 64, 6
    X = rng.standard_normal((M, K)).astype(F32)
    X[0] = 0.0                                # all zero: scale 0, Y = R + bias exactly
    X[1, 77] = 1.0e4 * np.abs(X[1]).max()     # one element 1e4 times the rest: they quantise to 0
    X[2, 7] = -2.0 * np.abs(X[2]).max()       # the largest magnitude is negative: -127, never -128
    s = F32(0.125)                            # ties: a * inv = j + 0.5 exactly (mx = 127 s, s a power of two)
    X[3] = 0.0
    X[3, 0], X[3, 1:127] = 127 * s, (np.arange(126) + 0.5) * s
    X[4] = -X[3]
    W, bias, R = operands(rng, M, K, N)
    Y, _, qx, sx = eng.dbg_dec_gemm_i8(W, bias, X=X, R=R, epi=RESID)
    q_ref, s_ref = quantize_rows(X)
    assert np.array_equal(qx, q_ref) and np.array_equal(bits(sx), bits(s_ref))
    check_y(pkg, Y, qx, sx, W, bias, R, RESID, M)
    assert sx[0] == 0.0 and not qx[0].any() and np.array_equal(bits(Y[0]), bits(R[0] + bias))
    assert qx[1, 77] == 127 and np.count_nonzero(qx[1]) == 1
    assert qx[2, 7] == -127 and qx.min() == -127
    assert list(qx[3, :127]) == [127] + list(range(1, 127)) and np.array_equal(qx[4], -qx[3])  # half away from zero


@pytest.mark.parametrize("case", ["K", "M0", "M129", "N", "ldy", "ldx", "combine", "logits", "ksplit", "bias", "X", "R", "ln_g"])
def test_launcher_refusals(pkg, eng, case):
    M, K, N = (0 if case == "M0" else 129 if case == "M129" else 4), (256 if case == "K" else 128), (40 if case == "N" else 32)
    W, bias, X = np.ones((N, K), F32), np.ones(N, F32), np.ones((M, 64 if case == "ldx" else K), F32)
    kw = dict(X=X, epi=BIAS)
    kw.update({"ldy": dict(ldy=16), "combine": dict(pro=2), "logits": dict(epi=3), "ksplit": dict(ksplit=2),
               "X": dict(X=None, pro=0, M=M), "R": dict(epi=RESID), "ln_g": dict(X=None, xin=X, ln_b=bias[:1].repeat(K))}.get(case, {}))
    with pytest.raises(pkg.WtError) as err:
        eng.dbg_dec_gemm_i8(W, None if case == "bias" else bias, **kw)
    assert err.value.code == 1


# ------------------------------------------------------------------------------------------- the engine, through the option ---
def test_engine_option(pkg, model):
    """The option takes 0 and 1 alone.  Off -> on -> off gives the first run back bit for bit (the graph keys); on differs
    from off at every step.  Then with logits_int8 as well, and a full-length call (twice: eager, then the captured
    segments): they run, and every id is the tie-rule argmax of the logits returned."""
    e, _, mel = model
    bf16 = e.get_option("bf16")
    for bad in (2, -1):
        with pytest.raises(pkg.WtError) as err:
            e.set_option("decoder_int8", bad)
        assert err.value.code == 1 and e.get_option("decoder_int8") == 0
    try:
        ids0, n0, _, lg0 = e.encdec_debug_batch(mel, steps_cap=6)
        assert list(n0) == [10, 10]
        e.set_forced_ids(ids0)  # both forms see the same ids
        e.set_option("decoder_int8", 1)
        assert e.get_option("decoder_int8") == 1
        _, _, _, lg_on = e.encdec_debug_batch(mel, steps_cap=6)
        e.set_forced_ids(None)
        e.set_option("logits_int8", 1)
        ids1, _, _, lg1 = e.encdec_debug_batch(mel, steps_cap=6)
        e.set_option("logits_int8", 0)
        e.set_option("full_bf16", bf16)
        e.set_option("max_positions", 40)
        full = [e.encdec_tokens_full(mel) for _ in range(2)]
        e.set_option("max_positions", 0)
        e.set_option("decoder_int8", 0)
        ids2, _, _, lg2 = e.encdec_debug_batch(mel, steps_cap=6)
    finally:
        e.set_forced_ids(None)
        for k in ("logits_int8", "decoder_int8", "max_positions", "full_bf16"):
            e.set_option(k, 0)
    assert np.array_equal(ids2, ids0) and np.array_equal(bits(lg2), bits(lg0))
    assert np.array_equal(full[0][0], full[1][0]) and np.array_equal(full[0][1], full[1][1]) and (full[0][1] > 4).all()
    for b in range(2):
        for s in range(6):
            assert (lg_on[b, s] != lg0[b, s]).any(), (b, s)
            assert ids1[b, 4 + s] == argmax_last(lg1[b, s]), (b, s)


# Largest |logit - float64 fake-quantised decoder's| measured on an MI355X over micro and tiny at 2 clips (4.53e-7, DESIGN
# section 38), times 4
ERR_BAR = 4 * 4.53e-7


@pytest.mark.parametrize("clips,absorbed", [(2, False), (32, True)])
def test_engine_against_the_float64_quantised_decoder(model, clips, absorbed):
    """fp32 storage: the logits against the float64 decoder that applies the same quantiser to the five matrices and to its
    own activation rows.  2 clips (the cached cross-attention: its kProCombine out-projection stays on dec_gemm, and the
    float64 decoder keeps that matrix in float64): the bar is 4 x the largest error measured and has to stay below a tenth
    of the distance between the fake-quantised and the unquantised float64 decoders on the same rows.
    32 clips (synchronous calls take the absorbed form from 32 clips on, all five matrices int8): the absorbed context is
    ~1e-5 off the float64 one, so now and then an element rounds to the other int8 step, and from there on a few per cent
    of the later elements do (measured 1.5e-7 without such a step, 2.5e-3 .. 1.5e-2 with: 0.07 .. 0.43 of the distance).
    A fake-quantised network is discontinuous, so that form is held to half the distance: a decoder that quantises one
    matrix more or fewer sits at 0.8 .. 0.95 of it (measured with this reference's cross-attention flag the wrong way)."""
    e, (dims, tensors), _ = model
    if e.get_option("bf16"):
        return  # (the comparison is stated for the fp32 storage mode)
    assert e.get_option("cross_absorb_active") == 1
    mel = np.random.default_rng(41).uniform(-1.0, 1.5, size=(clips,) + e.mel_shape).astype(F32)
    try:
        ids0, _, enc, _ = e.encdec_debug_batch(mel, steps_cap=6)
        e.set_forced_ids(ids0)
        e.set_option("decoder_int8", 1)
        _, _, _, lg_on = e.encdec_debug_batch(mel, steps_cap=6)
    finally:
        e.set_forced_ids(None)
        e.set_option("decoder_int8", 0)
    qweights = ref.quantized_weights(dims, tensors)
    errs, dists = [], []
    for b in (0, clips - 1):
        row = list(ids0[b, :9])
        lg_q, _ = ref.decoder_rows(dims, tensors, row, enc[b], qweights, cross_out=absorbed)
        lg_64, _ = ref.decoder_rows(dims, tensors, row, enc[b])
        errs.append(np.abs(lg_on[b] - lg_q[3:]).max())
        dists.append(np.abs(lg_q - lg_64)[3:].max())
        print(f"clip {b} of {clips}: largest error {errs[-1]:.3e}, fake-quantised to unquantised {dists[-1]:.3e}")
    if absorbed:
        assert all(err < dist / 2 for err, dist in zip(errs, dists)), (errs, dists)
    else:
        assert max(errs) <= ERR_BAR, errs
        assert ERR_BAR < min(dists) / 10, (ERR_BAR, dists)
