"""GPU (-m gpu): the int8 dynamic-range conv stem (option encoder_int8 = 2): the convolution kernels
and the clip maximum through their tap (bit for bit), the launcher's refusals, the engine through the option."""
import ctypes
import os

import numpy as np
import pytest

import decoder_int8_ref as dref
import encoder_conv_int8_ref as ref
import encoder_int8_ref
from conftest import GOLD
from test_gpu_decoder_step import eng, rel_err  # noqa: F401 (eng: the micro engine fixture)

pytestmark = pytest.mark.gpu
F32 = np.float32
BIAS, GELU, GELU_POS = 0, 1, 2
GUARD = F32(1.0e30)
# (stride, B, T_out, C_in, N): one row, micro's own shapes, one row past a tile and past two, every C_in, several column tiles
CASES = [(1, 1, 1, 80, 128), (1, 3, 200, 80, 128), (1, 2, 257, 80, 384), (1, 2, 130, 128, 128),
         (2, 1, 1, 128, 128), (2, 3, 100, 128, 128), (2, 2, 129, 384, 384), (2, 2, 257, 512, 512)]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check(eng, X, W, bias, pos, stride):
    """all three epilogues of one input: amax_in, Y (bias: bit for bit; GELU: the project's 3e-6 of the float64 GELU of the
    bit-exact pre-activation), amax_out against the returned Y, the guard rows.  Returns the pre-activation."""
    B, T_out = X.shape[0], X.shape[1] // stride
    qw, sw = ref.weights(W)
    pre, amax = zip(*(ref.conv(X[b], qw, sw, bias, stride) for b in range(B)))
    pre = np.stack(pre)
    for epi in (BIAS, GELU, GELU_POS):
        Y, amax_in, amax_out = eng.dbg_enc_conv_i8(X, W, bias, stride=stride, epi=epi, pos=pos)
        assert np.array_equal(bits(amax_in), bits(np.array(amax, F32)))
        if epi == BIAS:
            assert np.array_equal(bits(Y[:, :T_out]), bits(pre))
        else:
            want = dref.gelu64(pre) + (pos if epi == GELU_POS else 0.0)
            print(f"epilogue {epi}: largest deviation from the float64 GELU {rel_err(Y[:, :T_out], want):.3e}")
            assert rel_err(Y[:, :T_out], want) < 3e-6
        assert np.array_equal(bits(amax_out), bits(np.abs(Y[:, :T_out]).max(axis=(1, 2))))
        assert (Y[:, T_out:] == GUARD).all()
    return pre


@pytest.mark.parametrize("stride,B,T_out,C_in,N", CASES)
def test_conv(eng, stride, B, T_out, C_in, N):
    """the clips of a call are scaled by 1, 1e-3 and 50, so a wrong clip's scale or a read across a clip's pad row cannot
    hide; a clip's largest value sits in its first or its last row; the last clip of the 3-clip stride-1 case is all zero"""
    rng = np.random.default_rng(T_out * 7919 + C_in + stride)
    T_in = stride * T_out
    X = rng.standard_normal((B, T_in, C_in)).astype(F32)
    for b in range(B):
        X[b, (0, T_in - 1)[b & 1], rng.integers(C_in)] = (7.0, -7.0)[b & 1]
        X[b] *= F32((1.0, 1.0e-3, 50.0)[b])
    zero_clip = (stride, B) == (1, 3)
    if zero_clip:
        X[2] = 0.0
    W, bias = (rng.standard_normal((N, C_in, 3)) / 16).astype(F32), rng.standard_normal(N).astype(F32)
    pos = rng.standard_normal((T_out, N)).astype(F32)
    pre = check(eng, X, W, bias, pos, stride)
    if zero_clip:  # the epilogue of t = 0 exactly
        assert np.array_equal(bits(pre[2]), bits(np.broadcast_to(bias, pre[2].shape)))


def test_conv_accumulator_bound(eng):
    """all +127 against all +127 at C_in = 512, stride 2: acc = 127 * 127 * 1536 > 2^24 in the inner rows, one rounding"""
    rng = np.random.default_rng(5)
    X = np.full((1, 6, 512), 0.75, F32)
    W, bias = (rng.standard_normal((128, 512, 3)) / 16).astype(F32), rng.standard_normal(128).astype(F32)
    W[5] = 0.25
    check(eng, X, W, bias, rng.standard_normal((3, 128)).astype(F32), 2)
    q = np.full((6, 512), 127, np.int8)
    assert dref.acc_i32(ref.im2col(q, 2), ref.weights(W)[0])[1, 5] == 127 * 127 * 1536


@pytest.mark.parametrize("case", ["cin1", "cin2", "stride", "N", "B0", "T0", "bias", "pos", "epi", "X", "extent", "level3"])
def test_refusals(pkg, eng, case):
    """every refusal of the launcher that the tap can reach (it derives T_in from stride and T_out, so a T_in that is not
    2 T_out cannot be asked for) and the option's level 3"""
    if case == "level3":
        with pytest.raises(pkg.WtError) as err:
            eng.set_option("encoder_int8", 3)
        assert err.value.code == 1
        return
    if case in ("X", "extent"):  # (raw: no such array exists; the launcher's check touches no memory and comes first)
        a = np.zeros((8, 128), F32)
        fp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        T_out = 4 if case == "X" else 1 << 24
        rc = pkg.lib().wt_dbg_enc_conv_i8(eng.handle, 1, BIAS, 1, T_out, 80, 128, None if case == "X" else fp(a), fp(a), fp(a), None,
                                          fp(a), fp(a), fp(a))
        assert rc == 1 and (b"null operand" if case == "X" else b"32 bits") in pkg.lib().wt_last_error(eng.handle)
        return
    stride = {"cin2": 2, "stride": 3}.get(case, 1)
    C_in, N = (96 if case == "cin1" else 80), (192 if case == "N" else 128)
    X = np.ones((0 if case == "B0" else 1, 0 if case == "T0" else 4 * stride, C_in), F32)
    with pytest.raises(pkg.WtError) as err:
        eng.dbg_enc_conv_i8(X, np.ones((N, C_in, 3), F32), None if case == "bias" else np.ones(N, F32), stride=stride,
                            epi={"pos": GELU_POS, "epi": 3}.get(case, BIAS))
    assert err.value.code == 1 and "int8 encoder conv" in str(err.value)


def test_level_2_is_accepted(eng):
    """the test that fails without the feature"""
    eng.set_option("encoder_int8", 2)
    try:
        assert eng.get_option("encoder_int8") == 2
    finally:
        eng.set_option("encoder_int8", 0)


# ------------------------------------------------------------------------------------------- the engine, through the option ---
def test_engine_against_the_float64_quantised_encoder(pkg, assets):
    """micro, 2 clips, the mel of test_gpu_enc_gemm_i8.py.  D = the relative distance between the float64 encoder with stem
    and layers fake-quantised and the unquantised one; enc_out at level 2 lies within D / 2 of the former (DESIGN sections
    38, 39: the project's bar for a fake-quantised network) and differs from level 1's.  Then level 1 and level 0 on the
    same engine are bit for bit a fresh engine's.  With bf16 an encode at level 2 refuses."""
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
        enc = {}
        e.set_option("encoder_int8", 2)
        assert e.get_option("encoder_int8") == 2
        enc[2] = e.encdec_debug_batch(mel, steps_cap=6)[2]
        e.set_option("bf16", 1)
        with pytest.raises(pkg.WtError) as err:
            e.encdec_debug_batch(mel, steps_cap=6)
        assert err.value.code == 4
        e.set_option("bf16", 0)
        for level in (1, 0):
            e.set_option("encoder_int8", level)
            fresh.set_option("encoder_int8", level)
            enc[level] = e.encdec_debug_batch(mel, steps_cap=6)[2]
            assert np.array_equal(bits(enc[level]), bits(fresh.encdec_debug_batch(mel, steps_cap=6)[2]))
    finally:
        e.close()
        fresh.close()
    assert (enc[2] != enc[1]).any()
    for b in range(2):
        e_q, e_64 = ref.encoder_rows(dims, tensors, mel[b]), encoder_int8_ref.encoder_rows(dims, tensors, mel[b])
        D, err_q = rel_err(e_q, e_64), rel_err(enc[2][b], e_q)
        print(f"clip {b}: D = {D:.3e}, engine to fake-quantised {err_q:.3e} = {err_q / D:.3f} D")
        assert err_q < D / 2


def test_engine_tiny_golden_clips_decode(pkg, assets):
    """tiny, the golden's two clips at level 2: the call ends without error (a set non-finite flag is one) and the ids
    decode to text"""
    prefix, vocab = assets("tiny")
    g = np.load(os.path.join(GOLD, "model_tiny.npz"))
    mel = np.random.default_rng(int(g["mel_seed"])).uniform(-1.0, 1.5, size=(2, 80, 3000)).astype(F32)
    e = pkg.Engine(prefix, vocab, True)
    try:
        e.set_option("stop_at_eot", 0)
        e.set_option("encoder_int8", 2)
        ids, n = e.encdec_tokens_batch(mel)
        texts = [e.decode_bytes(ids[b, :n[b]], True) for b in range(2)]
    finally:
        e.close()
    print("ids equal to the golden's:", float((ids[:, :31] == g["ids"]).mean()))
    assert list(n) == [31, 31] and all(len(t) > 0 for t in texts)
