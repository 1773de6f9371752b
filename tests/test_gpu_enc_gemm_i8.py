"""GPU (-m gpu): the int8 dynamic-range encoder blocks (option encoder_int8): the GEMM and the row
quantiser through their taps (bit for bit), the launchers' refusals, the engine through the option."""
import ctypes
import os

import numpy as np
import pytest

import decoder_int8_ref as dref
import encoder_int8_ref as ref
from conftest import GOLD
from logits_int8_ref import boundary_distance, quantize_rows
from test_gpu_decoder_step import eng, ln64, rel_err  # noqa: F401 (eng: the micro engine fixture)

pytestmark = pytest.mark.gpu
F32 = np.float32
RESID, BIAS, GELU = 0, 1, 2
GUARD = F32(1.0e30)
SHAPES = [(1, 128, 128), (127, 128, 384), (129, 384, 1152), (300, 512, 512), (257, 1536, 384), (130, 2048, 512)]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_y(pkg, Y, qx, sx, W, bias, R, epi):
    """bias / residual: bit for bit; GELU: the project's 3e-6 of the float64 GELU of the bit-exact pre-activation; the four
    rows behind M untouched"""
    M = qx.shape[0]
    pre = dref.gemm(qx, sx, *pkg.quantize_rows_i8(W), bias, R if epi == RESID else None)
    if epi == GELU:
        assert rel_err(Y[:M], dref.gelu64(pre)) < 3e-6
    else:
        assert np.array_equal(bits(Y[:M]), bits(pre))
    assert (Y[M:] == GUARD).all()


@pytest.mark.parametrize("epi,in_place", [(BIAS, False), (RESID, False), (RESID, True), (GELU, False)])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_gemm(pkg, eng, M, K, N, epi, in_place):
    rng = np.random.default_rng(M * 7919 + K + epi)
    qx = rng.integers(-127, 128, (M, K)).astype(np.int8)
    sx = (10.0 ** rng.uniform(-2, 2, M)).astype(F32)
    W, bias, R = (rng.standard_normal((N, K)) / 16).astype(F32), rng.standard_normal(N).astype(F32), rng.standard_normal((M, N)).astype(F32)
    Y = eng.dbg_enc_gemm_i8(qx, sx, W, bias, R=R if epi == RESID else None, epi=epi, in_place=in_place)
    check_y(pkg, Y, qx, sx, W, bias, R, epi)


def test_gemm_accumulator_bound_and_zero_row(pkg, eng):
    """row 0 all +127 against weight row 5 all +127 at K = 2048: acc = 127 * 127 * 2048 > 2^24, one rounding; row 1 all
    zero with scale 0: R + bias exactly"""
    rng = np.random.default_rng(3)
    M, K, N = 3, 2048, 128
    qx = rng.integers(-127, 128, (M, K)).astype(np.int8)
    qx[0], qx[1] = 127, 0
    sx = np.array([0.37, 0.0, 1.5], F32)
    W, bias, R = (rng.standard_normal((N, K)) / 16).astype(F32), rng.standard_normal(N).astype(F32), rng.standard_normal((M, N)).astype(F32)
    W[5] = 0.25
    Y = eng.dbg_enc_gemm_i8(qx, sx, W, bias, R=R, epi=RESID)
    check_y(pkg, Y, qx, sx, W, bias, R, RESID)
    assert dref.acc_i32(qx, pkg.quantize_rows_i8(W)[0])[0, 5] == 127 * 127 * 2048
    assert np.array_equal(bits(Y[1]), bits(R[1] + bias))


def rows_with_edges(rng, M, K):
    """rows over four decades; from 9 rows on the first five are test_gpu_dec_gemm_i8.py::test_edge_rows'"""
    X = (rng.standard_normal((M, K)) * 10.0 ** rng.uniform(-2, 2, (M, 1))).astype(F32)
    if M >= 9:
        X[:5] = rng.standard_normal((5, K)).astype(F32)
        X[0] = 0.0                              # all zero: scale 0
        X[1, 77] = 1.0e4 * np.abs(X[1]).max()   # one element 1e4 times the rest: they quantise to 0
        X[2, 7] = -2.0 * np.abs(X[2]).max()     # the largest magnitude is negative: -127, never -128
        s = F32(0.125)                          # ties: a * inv = j + 0.5 exactly (mx = 127 s, s a power of two)
        X[3] = 0.0
        X[3, 0], X[3, 1:127] = 127 * s, (np.arange(126) + 0.5) * s
        X[4] = -X[3]
    return X


@pytest.mark.parametrize("source", ["f32", "planes"])
@pytest.mark.parametrize("K", [128, 384, 1536, 2048])
@pytest.mark.parametrize("M", [1, 9, 130])
def test_quantiser_rows(eng, M, K, source):
    X = rows_with_edges(np.random.default_rng(M * 31 + K), M, K)
    scale = F32(0.5)  # (the planes' power of two: the largest element, 1e4 x 4, stays inside fp16)
    if source == "planes":
        hi = (X * scale).astype(np.float16)
        lo = (X * scale - hi.astype(F32)).astype(np.float16)
        want = (hi.astype(F32) + lo.astype(F32)) / scale
    else:
        want = X
    qx, sx = eng.dbg_enc_quant_rows_i8(X, source, scale=scale)
    q_ref, s_ref = quantize_rows(want)
    assert np.array_equal(qx, q_ref) and np.array_equal(bits(sx), bits(s_ref))
    if M >= 9:
        assert sx[0] == 0.0 and not qx[0].any()
        assert qx[1, 77] == 127 and np.count_nonzero(qx[1]) == 1
        assert qx[2, 7] == -127 and qx.min() == -127
        assert list(qx[3, :127]) == [127] + list(range(1, 127)) and np.array_equal(qx[4], -qx[3])  # half away from zero


@pytest.mark.parametrize("K", [128, 384, 512])
@pytest.mark.parametrize("M", [9, 130])
def test_quantiser_layernorm(eng, M, K):
    """DESIGN section 37's bars for the same LayerNorm code: sx within 4 ulp of the float64 LayerNorm's scale, qx equal
    wherever a * inv is farther than 2e-3 from a rounding boundary and within 1 elsewhere"""
    rng = np.random.default_rng(M * 104729 + K)
    X = (rng.standard_normal((M, K)) * 2 + 0.5).astype(F32)
    g_, b_ = rng.standard_normal(K).astype(F32), rng.standard_normal(K).astype(F32)
    qx, sx = eng.dbg_enc_quant_rows_i8(X, "ln", ln_g=g_, ln_b=b_)
    ln = ln64(X, g_, b_)
    q_ref, s_ref = quantize_rows(ln.astype(F32))
    near = boundary_distance(ln) < 2e-3
    assert near.mean() < 0.01  # (a condition on the inputs)
    assert np.abs(sx.view(np.int32).astype(np.int64) - s_ref.view(np.int32)).max() <= 4
    diff = np.abs(qx.astype(np.int32) - q_ref)
    assert diff.max() <= 1 and not diff[~near].any()


@pytest.mark.parametrize("case", ["K", "M0", "N", "ldc", "bias", "sx", "R", "epi", "extent", "qK16", "qK2064", "qLnK", "qX", "qLnG"])
def test_launcher_refusals(pkg, eng, case):
    if case == "extent":  # (raw: no array of that pitch exists; the launcher's check touches no memory and comes first)
        a = np.zeros((5, 128), F32)
        vp, fp = ctypes.c_void_p, lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        rc = pkg.lib().wt_dbg_enc_gemm_i8(eng.handle, BIAS, 1, 128, 128, a.ctypes.data_as(vp), fp(a), fp(a), fp(a), None, 1 << 30, fp(a))
        assert rc == 1 and b"32 bits" in pkg.lib().wt_last_error(eng.handle)
        return
    with pytest.raises(pkg.WtError) as err:
        if case.startswith("q"):
            K = {"qK16": 24, "qK2064": 2064, "qLnK": 1024}.get(case, 128)
            X, g_ = None if case == "qX" else np.ones((4, K), F32), None if case == "qLnG" else np.ones(K, F32)
            eng.dbg_enc_quant_rows_i8(X, "ln" if "Ln" in case else "f32", ln_g=g_, ln_b=np.ones(K, F32), K=K)
        else:
            M, K, N = (0 if case == "M0" else 4), (256 if case == "K" else 128), (192 if case == "N" else 128)
            bias, sx = None if case == "bias" else np.ones(N, F32), None if case == "sx" else np.ones(M, F32)
            kw = {"ldc": dict(ldc=64), "R": dict(epi=RESID), "epi": dict(epi=3)}.get(case, {})
            eng.dbg_enc_gemm_i8(np.ones((M, K), np.int8), sx, np.ones((N, K), F32), bias, **kw)
    assert err.value.code == 1 and ("int8 row quantiser" if case.startswith("q") else "int8 encoder GEMM") in str(err.value)


# ------------------------------------------------------------------------------------------- the engine, through the option ---
def test_engine_against_the_float64_quantised_encoder(pkg, assets):
    """micro, 2 clips.  D = the relative distance between the float64 encoder that applies the same quantiser to the four
    matrices of every layer and to their input rows, and the unquantised float64 encoder; enc_out with the option on lies
    within D / 2 of the former (a fake-quantised network is discontinuous: DESIGN section 38 holds the absorbed decoder
    form to the same fraction).  Off again, enc_out is bit for bit a fresh engine's.  With bf16 an encode refuses."""
    from wtw import read_wtw
    prefix, vocab = assets("micro")
    dims, tensors = read_wtw(prefix + ".wtw")
    e, fresh = pkg.Engine(prefix, vocab, True), pkg.Engine(prefix, vocab, True)
    try:
        for x in (e, fresh):
            x.set_option("stop_at_eot", 0)
            x.set_prompt([3, 5, 7, 11])
            x.set_option("max_tokens", 9)
        mel = np.random.default_rng(43).uniform(-1.0, 1.5, size=(2,) + e.mel_shape).astype(F32)
        enc_fresh = fresh.encdec_debug_batch(mel, steps_cap=6)[2]
        e.set_option("encoder_int8", 1)
        assert e.get_option("encoder_int8") == 1
        enc_on = e.encdec_debug_batch(mel, steps_cap=6)[2]
        e.set_option("bf16", 1)
        with pytest.raises(pkg.WtError) as err:
            e.encdec_debug_batch(mel, steps_cap=6)
        assert err.value.code == 4
        e.set_option("bf16", 0)
        e.set_option("encoder_int8", 0)
        enc_off = e.encdec_debug_batch(mel, steps_cap=6)[2]
    finally:
        e.close()
        fresh.close()
    assert np.array_equal(bits(enc_off), bits(enc_fresh)) and (enc_on != enc_fresh).any()
    qweights = ref.quantized_weights(dims, tensors)
    for b in range(2):
        e_q, e_64 = ref.encoder_rows(dims, tensors, mel[b], qweights), ref.encoder_rows(dims, tensors, mel[b])
        D, err_q = rel_err(e_q, e_64), rel_err(enc_on[b], e_q)
        print(f"clip {b}: D = {D:.3e}, engine to fake-quantised {err_q:.3e} = {err_q / D:.3f} D, fresh engine to float64 {rel_err(enc_fresh[b], e_64):.3e}")
        assert err_q < D / 2


def test_engine_tiny_golden_clips_decode(pkg, assets):
    """tiny, the golden's two clips with the option on: the call ends without error (a set non-finite flag is one) and the
    ids decode to text"""
    prefix, vocab = assets("tiny")
    g = np.load(os.path.join(GOLD, "model_tiny.npz"))
    mel = np.random.default_rng(int(g["mel_seed"])).uniform(-1.0, 1.5, size=(2, 80, 3000)).astype(F32)
    e = pkg.Engine(prefix, vocab, True)
    try:
        e.set_option("stop_at_eot", 0)
        e.set_option("encoder_int8", 1)
        ids, n = e.encdec_tokens_batch(mel)
        texts = [e.decode_bytes(ids[b, :n[b]], True) for b in range(2)]
    finally:
        e.close()
    print("ids equal to the golden's:", float((ids[:, :31] == g["ids"]).mean()))
    assert list(n) == [31, 31] and all(len(t) > 0 for t in texts)
