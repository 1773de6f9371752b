"""A float64 encoder that runs the four Linear matrices of every layer through the int8 dynamic-range arithmetic of
DESIGN.md section 39: fp64_encoder.encoder_fp64's structure with a `lin` hook, as decoder_int8_ref.decoder_rows has it."""
import numpy as np

from decoder_int8_ref import gemm64
from fp64_encoder import _gelu, _ln
from logits_int8_ref import quantize_rows

_NAMES = [".attn.query.weight", ".attn.key.weight", ".attn.value.weight", ".attn.out.weight", ".mlp.0.weight", ".mlp.2.weight"]


def quantized_weights(dims, tensors):
    """name -> (qw, sw) of the matrices the option quantises (q | k | v row by row: fusing them changes nothing)"""
    return {f"encoder.blocks.{l}{n}": quantize_rows(tensors[f"encoder.blocks.{l}{n}"])
            for l in range(dims["n_audio_layer"]) for n in _NAMES}


def encoder_rows(dims, t, mel, qweights=None):
    """mel [n_mels][2 T] -> [T][d] float64.  With qweights every one of those matrices is int8 rows and each of its input
    rows goes through the same quantiser (of the float64 row rounded to float32); without, encoder_fp64's result."""
    f = lambda k: np.asarray(t[k], dtype=np.float64)
    H, L, T = dims["n_audio_head"], dims["n_audio_layer"], dims["n_audio_ctx"]

    def lin(h, name):
        return h @ f(name).T if qweights is None else gemm64(*quantize_rows(h), *qweights[name])

    x = np.asarray(mel, dtype=np.float64)
    T0 = x.shape[1]
    w1, w2 = f("encoder.conv1.weight"), f("encoder.conv2.weight")
    xp = np.pad(x, ((0, 0), (1, 1)))
    h = _gelu(sum(w1[:, :, k] @ xp[:, k:k + T0] for k in range(3)) + f("encoder.conv1.bias")[:, None])
    hp = np.pad(h, ((0, 0), (1, 1)))
    y = sum(w2[:, :, k] @ hp[:, k:k + T0:2][:, :T] for k in range(3)) + f("encoder.conv2.bias")[:, None]
    x = _gelu(y).T + f("encoder.positional_embedding")
    for l in range(L):
        p = f"encoder.blocks.{l}"
        a = _ln(x, f(p + ".attn_ln.weight"), f(p + ".attn_ln.bias"))
        q = lin(a, p + ".attn.query.weight") + f(p + ".attn.query.bias")
        k = lin(a, p + ".attn.key.weight")
        v = lin(a, p + ".attn.value.weight") + f(p + ".attn.value.bias")
        o = np.empty_like(q)
        for hh in range(H):
            sl = slice(64 * hh, 64 * hh + 64)
            s = q[:, sl] @ k[:, sl].T / 8.0
            s = np.exp(s - s.max(-1, keepdims=True))
            o[:, sl] = (s / s.sum(-1, keepdims=True)) @ v[:, sl]
        x = x + (lin(o, p + ".attn.out.weight") + f(p + ".attn.out.bias"))
        m = _gelu(lin(_ln(x, f(p + ".mlp_ln.weight"), f(p + ".mlp_ln.bias")), p + ".mlp.0.weight") + f(p + ".mlp.0.bias"))
        x = x + (lin(m, p + ".mlp.2.weight") + f(p + ".mlp.2.bias"))
    return _ln(x, f("encoder.ln_post.weight"), f("encoder.ln_post.bias"))
