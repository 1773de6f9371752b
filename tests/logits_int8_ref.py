"""numpy restatement of the int8 dynamic-range logits head."""
import numpy as np

import align_ref

F32 = np.float32


def quantize_rows(a):
    """a [rows][K] -> (q int8, scale float32): mx = max |a_k|, scale = mx / 127, inv = 127 / mx (both 0 at mx == 0),
    q = clamp(round-half-away-from-zero(a * inv), -127, 127), every step in fp32 (v - trunc(v) is exact)."""
    a = np.asarray(a, F32)
    mx = np.abs(a).max(axis=1)
    safe = np.where(mx > 0, mx, F32(1))
    scale = np.where(mx > 0, mx / F32(127), F32(0)).astype(F32)
    inv = np.where(mx > 0, F32(127) / safe, F32(0)).astype(F32)
    v = a * inv[:, None]
    t = np.trunc(v)
    r = t + np.sign(v) * (np.abs(v - t) >= F32(0.5))
    return np.clip(r, -127, 127).astype(np.int8), scale


def logits(qx, sx, qw, sw):
    """the head's arithmetic; the fp32 matrix product of the int8 values is exact (every partial sum is below 2^24)"""
    acc = qx.astype(F32) @ qw.astype(F32).T
    return (acc * sx.astype(F32)[:, None]) * sw.astype(F32)[None, :]


def boundary_distance(ln):
    """distance of the float64 value a * inv from the nearest rounding boundary (j + 0.5), per element of ln [M][K]"""
    t = np.abs(ln) * (127.0 / np.abs(ln).max(axis=1))[:, None]
    return np.abs(t - np.floor(t) - 0.5)


def worst_case(ln, E):
    """per (row, column) the spec's worst distance from ln . E^T: each factor is off by at most half its step"""
    sx, sw = np.abs(ln).max(axis=1) / 127.0, np.abs(E).max(axis=1) / 127.0
    return (0.5 * np.outer(np.abs(ln).sum(axis=1), sw) + 0.5 * np.outer(sx, np.abs(E).sum(axis=1))
            + ln.shape[1] * np.outer(sx, sw) / 4.0)


def decoder_rows(dims, tensors, row, enc):
    """align_ref.decoder_forward's float64 logits [L][V] and final-LayerNorm rows [L][d]: the logits of d unit rows
    appended to the tied embedding (no id of `row` reaches them)"""
    d, V = dims["n_text_state"], dims["n_vocab"]
    t = dict(tensors)
    t["decoder.token_embedding.weight"] = np.concatenate([np.asarray(t["decoder.token_embedding.weight"], np.float64), np.eye(d)])
    out, _ = align_ref.decoder_forward(dims, t, row, enc)
    return out[:, :V], out[:, V:]
