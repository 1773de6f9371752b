"""numpy restatement of option cross_int8: the value the planes hold, the two quantisers, the
attention on the dequantised operands in float64, and a float64 decoder whose cross-attention runs through them."""
import numpy as np

import align_ref
from logits_int8_ref import F32, quantize_rows


def planes_value(E, e_scale):
    """what the default kernel reconstructs from the two fp16 planes of E * e_scale: (hi + lo) * (1 / e_scale) in float32"""
    v = np.asarray(E, F32) * F32(e_scale)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(F32)).astype(np.float16)
    return (hi.astype(F32) + lo.astype(F32)) * F32(1.0 / e_scale)


def bf16_value(E):
    """E rounded to bf16 (nearest even), as float32: the bf16 storage mode's plane"""
    u = np.ascontiguousarray(E, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)


def quantize_e(x):
    """x [..., T][d] float32 -> (qe int8 of the same shape, se float32 [..., T]): one scale per key row"""
    q, s = quantize_rows(np.asarray(x, F32).reshape(-1, x.shape[-1]))
    return q.reshape(x.shape), s.reshape(x.shape[:-1])


def quantize_q(qp, H):
    """qp [rows][H * d] -> (qq int8 [rows][H][d], sq float32 [rows][H]): one scale per query column (row, head)"""
    rows, d = qp.shape[0], qp.shape[1] // H
    q, s = quantize_rows(np.asarray(qp, F32).reshape(rows * H, d))
    return q.reshape(rows, H, d), s.reshape(rows, H)


def attend(Q, E):
    """float64: Q [n][H][d] (log2 domain), E [T][d] -> the normalised contexts sum_j softmax2_j(Q . e_j) e_j [n][H][d]"""
    S = np.einsum("nhd,td->nht", Q, E)
    P = np.exp2(S - S.max(axis=2, keepdims=True))
    return (P / P.sum(axis=2, keepdims=True)) @ E


def clip_out(qe, se, qq, sq, wv, bv):
    """one clip on the dequantised operands: qe [T][d], se [T], qq [n][H][d], sq [n][H] -> out [n][H * 64] in float64"""
    n, H, d = qq.shape
    c = attend(qq.astype(np.float64) * sq.astype(np.float64)[..., None], qe.astype(np.float64) * se.astype(np.float64)[:, None])
    out = np.einsum("hjd,nhd->nhj", np.asarray(wv, np.float64).reshape(H, 64, d), c) + np.asarray(bv, np.float64).reshape(H, 64)
    return out.reshape(n, H * 64)


def decoder_logits(dims, tensors, row, enc, quantised):
    """align_ref.decoder_forward's float64 decoder on one id row, cross-attention in the absorbed form (q'_h = c0 Wk_h^T q_h
    against enc itself, Wv_h on the context); `quantised`: q' and enc go through the quantisers above.  Logits [L][V]."""
    t = {k: np.asarray(v, np.float64) for k, v in tensors.items() if k.startswith("decoder.")}
    H, d, L = dims["n_text_head"], dims["n_text_state"], len(row)
    ln, E = align_ref._ln, np.asarray(enc, np.float64)
    if quantised:
        qe, se = quantize_e(np.asarray(enc, F32))
        E = qe.astype(np.float64) * se.astype(np.float64)[:, None]
    x = t["decoder.token_embedding.weight"][np.asarray(row)] + t["decoder.positional_embedding"][:L]
    causal = np.triu(np.ones((L, L), bool), 1)
    for l in range(dims["n_text_layer"]):
        b = f"decoder.blocks.{l}"
        h = ln(x, t[b + ".attn_ln.weight"], t[b + ".attn_ln.bias"])
        q, k = h @ t[b + ".attn.query.weight"].T + t[b + ".attn.query.bias"], h @ t[b + ".attn.key.weight"].T
        v = h @ t[b + ".attn.value.weight"].T + t[b + ".attn.value.bias"]
        att = np.zeros_like(x)
        for hh in range(H):
            s = slice(64 * hh, 64 * hh + 64)
            sc = q[:, s] @ k[:, s].T / 8.0
            sc[causal] = -np.inf
            p = np.exp(sc - sc.max(axis=-1, keepdims=True))
            att[:, s] = (p / p.sum(axis=-1, keepdims=True)) @ v[:, s]
        x = x + att @ t[b + ".attn.out.weight"].T + t[b + ".attn.out.bias"]
        h = ln(x, t[b + ".cross_attn_ln.weight"], t[b + ".cross_attn_ln.bias"])
        q = (h @ t[b + ".cross_attn.query.weight"].T + t[b + ".cross_attn.query.bias"]).reshape(L, H, 64)
        qp = np.einsum("lhj,hjd->lhd", q, t[b + ".cross_attn.key.weight"].reshape(H, 64, d)) * (np.log2(np.e) / 8.0)
        if quantised:
            qq, sq = quantize_q(qp.reshape(L, H * d).astype(F32), H)
            qp = qq.astype(np.float64) * sq.astype(np.float64)[..., None]
        c = attend(qp, E)
        att = np.einsum("hjd,lhd->lhj", t[b + ".cross_attn.value.weight"].reshape(H, 64, d), c).reshape(L, d)
        x = x + (att + t[b + ".cross_attn.value.bias"]) @ t[b + ".cross_attn.out.weight"].T + t[b + ".cross_attn.out.bias"]
        h = ln(x, t[b + ".mlp_ln.weight"], t[b + ".mlp_ln.bias"])
        h = h @ t[b + ".mlp.0.weight"].T + t[b + ".mlp.0.bias"]
        x = x + (0.5 * h * (1.0 + align_ref._erf(h / np.sqrt(2.0)))) @ t[b + ".mlp.2.weight"].T + t[b + ".mlp.2.bias"]
    return ln(x, t["decoder.ln.weight"], t["decoder.ln.bias"]) @ t["decoder.token_embedding.weight"].T
