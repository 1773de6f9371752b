"""numpy restatement of the int8 dynamic-range conv stem and a float64 encoder that runs the stem
through it and the layers through encoder_int8_ref's.  One input scale per clip is quantize_rows of the clip as ONE row;
the contraction is decoder_int8_ref.gemm over the im2col of the quantised clip with that scale on every row."""
import numpy as np

import encoder_int8_ref
from decoder_int8_ref import gelu64, gemm, gemm64
from logits_int8_ref import F32, quantize_rows


def weights(W):
    """W [N][C_in][3] -> (qw int8 [N][3 C_in] in the implicit GEMM's order [tap C_in + ci], sw [N])"""
    W = np.asarray(W, F32)
    return quantize_rows(W.transpose(0, 2, 1).reshape(W.shape[0], -1))


def im2col(q, stride):
    """q [T_in][C_in] -> [T_in / stride][3 C_in]: output row t holds the padded rows stride t .. stride t + 2"""
    qp, n = np.pad(q, ((1, 1), (0, 0))), q.shape[0] // stride * stride
    return np.concatenate([qp[j:j + n:stride] for j in range(3)], axis=1)


def conv(X, qw, sw, bias, stride, f64=False):
    """one clip X [T_in][C_in] -> (t + bias [T_out][N], amax): float32 with every step rounded on its own (the kernel), or
    the same integers with the scales applied in float64 (the float64 encoder)"""
    X = np.asarray(X, F32)
    q, s = quantize_rows(X.reshape(1, -1))
    A = im2col(q.reshape(X.shape), stride)
    sx = np.full(A.shape[0], s[0], F32)
    y = gemm64(A, sx, qw, sw) + np.asarray(bias, np.float64) if f64 else gemm(A, sx, qw, sw, np.asarray(bias, F32))
    return y, np.abs(X).max()


def encoder_rows(dims, t, mel):
    """mel [n_mels][2 T] -> [T][d] float64 with the stem AND the layers fake-quantised.  The layers are
    encoder_int8_ref.encoder_rows': it is handed zero convolutions (GELU(0) = 0) and this stem's output as its positional
    table, so its residual stream starts at exactly that output."""
    f = lambda k: np.asarray(t[k], np.float64)
    h = gelu64(conv(np.asarray(mel).T, *weights(t["encoder.conv1.weight"]), f("encoder.conv1.bias"), 1, True)[0])
    x = gelu64(conv(h, *weights(t["encoder.conv2.weight"]), f("encoder.conv2.bias"), 2, True)[0]) + f("encoder.positional_embedding")
    t2 = dict(t)
    for k in ("encoder.conv1.weight", "encoder.conv1.bias", "encoder.conv2.weight", "encoder.conv2.bias"):
        t2[k] = np.zeros_like(t[k])
    t2["encoder.positional_embedding"] = x
    return encoder_int8_ref.encoder_rows(dims, t2, mel, encoder_int8_ref.quantized_weights(dims, t))
