"""CPU: the numpy restatement of the int8 decoder blocks (decoder_int8_ref.py) checked against plain
float64 arithmetic, and the distance between the fake-quantised and the unquantised float64 decoders on micro: what lets
tests/test_gpu_dec_gemm_i8.py tell int8 arithmetic from fp arithmetic at all."""
import numpy as np
import pytest

import decoder_int8_ref as ref
from logits_int8_ref import quantize_rows


@pytest.mark.parametrize("M,K,N", [(5, 128, 96), (33, 2048, 64)])
def test_gemm_is_the_product_of_the_dequantised_operands(M, K, N):
    rng = np.random.default_rng(K + M)
    (qx, sx), (qw, sw) = quantize_rows(rng.standard_normal((M, K)) * 3), quantize_rows(rng.standard_normal((N, K)) / 16)
    want = (qx * sx.astype(np.float64)[:, None]) @ (qw * sw.astype(np.float64)[:, None]).T
    got = ref.gemm64(qx, sx, qw, sw)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the float32 form rounds three times (the conversion at |acc| >= 2^24 and two products), the sum with the bias once
    bias = rng.standard_normal(N).astype(np.float32)
    f32 = ref.gemm(qx, sx, qw, sw, bias)
    assert f32.dtype == np.float32
    assert (np.abs(f32 - (want + bias)) <= 3 * 2.0 ** -24 * np.abs(want) + 2.0 ** -24 * np.abs(want + bias) + 1e-30).all()


def test_fake_quantised_decoder_is_far_from_the_unquantised_one(pkg, assets):
    from wtw import read_wtw
    prefix, _ = assets("micro")
    dims, tensors = read_wtw(prefix + ".wtw")
    assert "wt_dbg_dec_gemm_i8" in pkg.DEBUG_SYMBOLS and pkg.lib().wt_dbg_dec_gemm_i8
    enc = np.random.default_rng(3).standard_normal((dims["n_audio_ctx"], dims["n_text_state"]))
    row = [3, 5, 7, 11, 100, 200, 300, 400, 500]
    lg, _ = ref.decoder_rows(dims, tensors, row, enc)
    lg_q, _ = ref.decoder_rows(dims, tensors, row, enc, ref.quantized_weights(dims, tensors))
    dist = np.abs(lg_q - lg)[3:].max(axis=1)
    print("micro: |fake-quantised - unquantised| per row", dist)
    assert dist.min() > 10 * 1e-4  # the fp32 path's bar is 1e-4
