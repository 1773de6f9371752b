"""numpy restatement of the int8 dynamic-range decoder-block GEMM and a float64 decoder that
runs the five Linear matrices of every layer through it."""
import numpy as np

import align_ref
from logits_int8_ref import F32, quantize_rows


def acc_i32(qx, qw):
    """sum_k qx qw, exact (|acc| <= 127 * 127 * 2048 < 2^25; the fp64 product holds every partial sum)"""
    return (qx.astype(np.float64) @ qw.astype(np.float64).T).astype(np.int32)


def gemm(qx, sx, qw, sw, bias, R=None):
    """the kernel's arithmetic in float32, every product and sum rounded on its own: t = ((float)acc * sx) * sw, then
    t + bias, or R + (t + bias); GELU is applied to this pre-activation"""
    t = (acc_i32(qx, qw).astype(F32) * sx.astype(F32)[:, None]) * sw.astype(F32)[None, :]
    v = t + bias.astype(F32)[None, :]
    return v if R is None else R.astype(F32) + v


def gemm64(qx, sx, qw, sw):
    """the same product with the scales applied in float64: what the float64 decoder below uses"""
    return acc_i32(qx, qw).astype(np.float64) * sx.astype(np.float64)[:, None] * sw.astype(np.float64)[None, :]


def gelu64(v):
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1.0 + align_ref._erf(v / np.sqrt(2.0)))


def embedding_rows(ids, pos, M, tok_emb, pos_emb, pos_start=None):
    """row p * B + b = tok_emb[ids[b][pos + p]] + pos_emb[clamp(pos + p - pos_start[b])] in float32 (one rounding)"""
    B = ids.shape[0]
    p, b = np.arange(M) // B, np.arange(M) % B
    pr = pos + p if pos_start is None else np.clip(pos + p - np.asarray(pos_start)[b], 0, pos_emb.shape[0] - 1)
    return tok_emb[ids[b, pos + p]].astype(F32) + pos_emb[pr].astype(F32)


def quantized_weights(dims, tensors):
    """name -> (qw, sw) of the five matrices per layer the option quantises (q | k | v row by row: fusing them changes nothing)"""
    names = [".attn.query.weight", ".attn.key.weight", ".attn.value.weight", ".attn.out.weight", ".cross_attn.out.weight",
             ".mlp.0.weight", ".mlp.2.weight"]
    return {f"decoder.blocks.{l}{n}": quantize_rows(tensors[f"decoder.blocks.{l}{n}"])
            for l in range(dims["n_text_layer"]) for n in names}


def decoder_rows(dims, tensors, row, enc, qweights=None, cross_out=True, want_logits=True):
    """align_ref.decoder_forward's float64 decoder on one id row, returning (logits [L][V], final-LayerNorm rows [L][d]).
    With qweights (quantized_weights) the five matrices are int8 rows and each of their input rows goes through the same
    quantiser (of the float64 row rounded to float32); cross_out False keeps the cross-attention out-projection in
    float64 (the cached cross-attention form); want_logits False returns None for the logits (a step-by-step decode
    takes the head of its last row alone)."""
    t = {k: np.asarray(v, np.float64) for k, v in tensors.items() if k.startswith("decoder.")}
    H, L = dims["n_text_head"], len(row)
    ln, enc = align_ref._ln, np.asarray(enc, np.float64)

    def lin(h, name, quant=True):
        if qweights is None or not quant:
            return h @ t[name].T
        return gemm64(*quantize_rows(h), *qweights[name])

    def attend(q, k, v, mask):
        att = np.zeros_like(q)
        for hh in range(H):
            s = slice(64 * hh, 64 * hh + 64)
            sc = q[:, s] @ k[:, s].T / 8.0
            if mask is not None:
                sc[mask] = -np.inf
            p = np.exp(sc - sc.max(axis=-1, keepdims=True))
            att[:, s] = (p / p.sum(axis=-1, keepdims=True)) @ v[:, s]
        return att

    x = t["decoder.token_embedding.weight"][np.asarray(row)] + t["decoder.positional_embedding"][:L]
    causal = np.triu(np.ones((L, L), bool), 1)
    for l in range(dims["n_text_layer"]):
        b = f"decoder.blocks.{l}"
        h = ln(x, t[b + ".attn_ln.weight"], t[b + ".attn_ln.bias"])
        att = attend(lin(h, b + ".attn.query.weight") + t[b + ".attn.query.bias"], lin(h, b + ".attn.key.weight"),
                     lin(h, b + ".attn.value.weight") + t[b + ".attn.value.bias"], causal)
        x = x + (lin(att, b + ".attn.out.weight") + t[b + ".attn.out.bias"])
        h = ln(x, t[b + ".cross_attn_ln.weight"], t[b + ".cross_attn_ln.bias"])
        att = attend(h @ t[b + ".cross_attn.query.weight"].T + t[b + ".cross_attn.query.bias"],
                     enc @ t[b + ".cross_attn.key.weight"].T,
                     enc @ t[b + ".cross_attn.value.weight"].T + t[b + ".cross_attn.value.bias"], None)
        x = x + (lin(att, b + ".cross_attn.out.weight", cross_out) + t[b + ".cross_attn.out.bias"])
        h = ln(x, t[b + ".mlp_ln.weight"], t[b + ".mlp_ln.bias"])
        h = gelu64(lin(h, b + ".mlp.0.weight") + t[b + ".mlp.0.bias"])
        x = x + (lin(h, b + ".mlp.2.weight") + t[b + ".mlp.2.bias"])
    x = ln(x, t["decoder.ln.weight"], t["decoder.ln.bias"])
    return (x @ t["decoder.token_embedding.weight"].T if want_logits else None), x
