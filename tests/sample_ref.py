"""Reference temperature sampling and fall-back: the definitions of DESIGN.md section 19 (options temperature,
temperature_fallback) restated in numpy over any next-token logits function.

  token   = argmax over the allowed ids i of k_i = z_i * inv_t + g_i, the larger id on equal keys; T = 0: k_i = z_i
  inv_t   = fp32(1) / fp32(T), the value the kernels multiply by
  g_i     = -log(-log u_i) in float64 from the SAME u_i the kernels use
  u_i     = ((x >> 9) + 0.5) * 2^-23 (exact in fp32), x = word (i & 3) of Philox4x32-10 under the counter
            (i >> 2, pos, clip, attempt) and the key (seed & 0xffffffff, seed >> 32)
  allowed = the whole vocabulary, or with timestamps the set rules 1 .. 5 of ts_ref leave (rule 5 on the untempered z)
  scores  = scores_ref's, from the untempered logits over the set the step chose from

Every step records the gap between the best and second-best key and the bar under which the fp32 kernels may order
the two differently (key_bar)."""
from __future__ import annotations

import math
import zlib

import numpy as np

import scores_ref
import ts_ref

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays."""
    c = [np.asarray(x, np.uint64) & MASK for x in np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in counter])]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)  # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x.astype(np.uint32) for x in c]


def words(V, pos, clip, attempt, seed):
    """The 32-bit word of every id 0 .. V - 1: one Philox call per quad of ids."""
    nq = (V + 3) // 4
    out = philox4x32_10((np.arange(nq), pos, clip, attempt), (seed & MASK, (seed >> 32) & MASK))
    return np.stack(out, axis=1).reshape(-1)[:V]


def uniform_of(x):
    """u as float32; the arithmetic is exact in fp32 (23 bits + a half, times a power of two)."""
    u = ((np.asarray(x, np.uint32) >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    return u


def gumbel_of(u):
    return -np.log(-np.log(np.asarray(u, np.float32).astype(np.float64)))


def inv_t_of(T):
    T = np.float32(T)
    return np.float32(0.0) if T == 0 else np.float32(1.0) / T


def temperature_of_milli(milli):
    """The temperature the engine forms from an option in thousandths."""
    return np.float32(milli) / np.float32(1000.0)


def key_bar(k, g):
    """How far the kernel's fp32 key of one id may lie from the float64 key k = z * inv_t + g (g its Gumbel term).
    logf on gfx950 is the hardware's base-2 logarithm (v_log_f32, within 1 ulp) times ln 2 in split precision: one ulp of
    log2 x is at most 2 ln 2 = 1.39 ulp of the product (which may lie one binade lower), and the product is rounded
    once more, so logf is within 2 ulp.  a = logf(u) therefore carries a relative error of 2 * 2^-23, which moves
    log(-a) by as much; the outer logf adds 2 ulp of |g|; the fmaf rounds once: half an ulp of |k| (z * inv_t is exact
    inside it, and u is exact)."""
    return 2.0 * 2.0 ** -23 + 2.0 * float(np.spacing(np.float32(abs(g)))) + 0.5 * float(np.spacing(np.float32(abs(k))))


def allowed_mask(z, g, eot, beg, max_initial=50, timestamps=False, check=False):
    """(mask of the ids the step may choose, {L, M, gap_lm, mass} or None).  Rules 1 .. 4 are scores_ref.intervals, rule 5
    is decided as ts_ref.step decides it (L by the same formula); check = True runs ts_ref.step beside it and asserts that
    the two agree."""
    z = np.asarray(z, np.float32)
    V = z.size
    if not timestamps:
        return np.ones(V, bool), None
    t_lo, t_hi, s_lo, s_hi = scores_ref.intervals(list(g), V, eot, beg, max_initial)
    mask = np.zeros(V, bool)
    L = M = None
    if s_lo <= s_hi:
        L = scores_ref.logsumexp64(z[s_lo:s_hi + 1])
    if t_lo <= t_hi:
        M = float(z[t_lo:t_hi + 1].max())
    mass = L is not None and M is not None and L > M
    if t_lo <= t_hi and not mass:
        mask[t_lo:t_hi + 1] = True
    if s_lo <= s_hi:
        mask[s_lo:s_hi + 1] = True
    info = {"L": L, "M": M, "mass": mass,
            "gap_lm": math.inf if L is None or M is None else (0.0 if L == M else abs(L - M))}
    if check:
        tok, ref = ts_ref.step(z, list(g), eot, beg, max_initial)
        assert mask[tok] and ("mass" in ref["fired"]) == mass and ref["gap_lm"] == info["gap_lm"]
        assert ref["L"] == L and ref["M"] == M
    return mask, info


def step(z, g, T, seed=0, pos=0, clip=0, attempt=0, eot=0, beg=0, max_initial=50, timestamps=False, check=False):
    """One sampling step on the fp32 logits z behind the generated ids g.  Returns (token, info): key (float64), gap (to
    the second-best key; inf with one allowed id, 0 on equal keys), bar (the sum of key_bar over the two), key_bar (of the
    winner alone), lp (the token's log-probability as scores_ref.token_logprob defines it), L, M, gap_lm."""
    z = np.asarray(z, np.float32)
    mask, tsi = allowed_mask(z, g, eot, beg, max_initial, timestamps, check)
    idx = np.flatnonzero(mask)
    z64 = z[idx].astype(np.float64)
    inv_t = inv_t_of(T)
    if inv_t == 0:
        k, gum = z64, np.zeros(idx.size)
    else:
        gum = gumbel_of(uniform_of(words(z.size, pos, clip, attempt, seed)[idx]))
        with np.errstate(invalid="ignore"):
            k = z64 * np.float64(inv_t) + gum
    best = int(np.flatnonzero(k == k.max())[-1])  # the larger id on equal keys
    den = scores_ref.logsumexp64(z[idx])  # scores_ref.token_logprob's value: the untempered logits over the allowed set
    info = {"key": float(k[best]), "gap": math.inf, "bar": 0.0, "lp": -math.inf if den == -math.inf else float(z64[best] - den),
            "key_bar": key_bar(k[best], gum[best]) if inv_t != 0 and np.isfinite(k[best]) else 0.0,
            "L": tsi["L"] if tsi else None, "M": tsi["M"] if tsi else float(z.max()),
            "gap_lm": tsi["gap_lm"] if tsi else math.inf}
    if idx.size > 1:
        rest = np.delete(np.arange(idx.size), best)
        second = int(rest[np.argmax(k[rest])])
        info["gap"] = 0.0 if k[second] == k[best] else float(k[best] - k[second])
        if inv_t != 0 and np.isfinite(k[best]):
            info["bar"] = key_bar(k[best], gum[best]) + (key_bar(k[second], gum[second]) if np.isfinite(k[second]) else 0.0)
    return int(idx[best]), info


def decode(logits_fn, prompt, max_pos, eot, nosp, T, seed=0, clip=0, attempt=0, beg=0, timestamps=False, max_initial=50,
           stop_at_eot=True, check=False):
    """Decoding at temperature T over positions 0 .. max_pos - 1 with scores, in the style of scores_ref.decode.  Returns
    its dict plus infos (step()'s info per generated id)."""
    ids = [int(i) for i in prompt]
    n_prompt = len(ids)
    nsp = scores_ref.no_speech_prob(logits_fn(ids[:1]), nosp)
    lps, infos = [], []
    while len(ids) <= max_pos:
        z = np.asarray(logits_fn(ids), np.float32)
        g = ids[n_prompt:]
        tok, info = step(z, g, T, seed, len(ids) - 1, clip, attempt, eot, beg, max_initial, timestamps, check)
        lps.append(info["lp"])
        infos.append(info)
        ids.append(tok)
        if stop_at_eot and tok == eot:
            break
    s = float(np.sum(np.asarray(lps, np.float64)))
    return {"ids": ids, "lps": lps, "sum": s, "n": len(lps), "avg": s / len(lps), "no_speech_prob": nsp, "infos": infos,
            "temperature": float(np.float32(T))}


def first_indecisive(infos, extra=0.0):
    """Index of the first step whose key gap is at or below its bar + extra, or whose rule-5 gap is at or below extra
    (None: the clip is decisive), in the pattern of ts_ref.first_indecisive."""
    for s, info in enumerate(infos):
        if info["gap"] <= info["bar"] + extra or info["gap_lm"] <= extra:
            return s
    return None


# ---- fall-back (Whisper's decode_with_fallback) ----
def schedule(t0_milli, increment_milli=200, fallback=True):
    """Temperatures in thousandths: t0, t0 + increment, ... up to 1000 inclusive (t0 alone without fall-back)."""
    if not fallback:
        return [int(t0_milli)]
    return list(range(int(t0_milli), 1001, int(increment_milli)))


def compression_ratio(text: bytes) -> float:
    """len(text) / len(zlib.compress(text)) in float64 (the engine reports it rounded to fp32), 0 for an empty text."""
    if not text:
        return 0.0
    return len(text) / len(zlib.compress(text))


def needs_fallback(ratio, avg, nsp, compression_ratio_threshold=2.4, logprob_threshold=-1.0, no_speech_threshold=0.6):
    """Whisper's rule; a threshold of None is off."""
    need = False
    if compression_ratio_threshold is not None and ratio > compression_ratio_threshold:
        need = True
    if logprob_threshold is not None and avg < logprob_threshold:
        need = True
    if (no_speech_threshold is not None and nsp > no_speech_threshold and logprob_threshold is not None
            and avg < logprob_threshold):
        need = False  # silence
    return need


def decode_with_fallback(decode_at, text_of, temps_milli, compression_ratio_threshold=2.4, logprob_threshold=-1.0,
                         no_speech_threshold=0.6):
    """decode_at(attempt, T) -> decode()'s dict; text_of(ids) -> bytes.  Returns the kept result with temperature_milli,
    attempts, needs_fallback (of the kept result) and compression_ratio added."""
    out = None
    for attempt, milli in enumerate(temps_milli):
        r = decode_at(attempt, temperature_of_milli(milli))
        ratio = compression_ratio(text_of(r["ids"]))
        need = needs_fallback(ratio, r["avg"], r["no_speech_prob"], compression_ratio_threshold, logprob_threshold,
                              no_speech_threshold)
        out = dict(r, temperature_milli=int(milli), attempts=attempt + 1, needs_fallback=bool(need), compression_ratio=ratio)
        if not need:
            break
    return out
