"""Reference decode confidence: the definitions of DESIGN.md section 15 (option scores) restated in Python over any
next-token logits function — the CPU oracle (ts_model.logits_fn) for the parity tests, hand-made tables for the kernel
tests.

  lp(step)        = z[tok] - logsumexp(z[i] : i allowed at that step), float64 from the fp32 logits z; without
                    timestamps every id is allowed, with them the set the step chose from: rules 1 .. 4 of ts_ref, then
                    rule 5 (L > M: only the allowed timestamps remain).  A denominator of -inf gives -inf, never NaN.
  sum_logprob     = sum of lp over the ids a clip generated, the EOT that ended it included; n_generated = their number
  avg_logprob     = sum_logprob / n_generated
  no_speech_prob  = exp(z0[nosp] - logsumexp(z0)), z0 = the logits behind the first prompt id (sot) alone, unfiltered
  skipped         = no_speech_prob > no_speech_threshold and not avg_logprob > logprob_threshold (Whisper's rule)"""
from __future__ import annotations

import math

import numpy as np

import ts_ref


def logsumexp64(v):
    """float64 log-sum-exp of the fp32 values v; -inf for an empty v or one that is all -inf."""
    v = np.asarray(v, np.float32).astype(np.float64)
    if v.size == 0:
        return -math.inf
    m = v.max()
    if m == -math.inf:
        return -math.inf
    return float(m + math.log(np.exp(v - m).sum()))


def intervals(g, V, eot, beg, max_initial=50):
    """Rules 1 .. 4 as two inclusive id intervals (t_lo, t_hi, s_lo, s_hi) behind the generated ids g; lo > hi: empty."""
    n = len(g)
    last_ts = n >= 1 and g[-1] >= beg
    pen_ts = n < 2 or g[-2] >= beg
    t_lo, t_hi, s_lo, s_hi = 0, eot, beg, V - 1
    if last_ts and pen_ts:
        s_lo = V
    if last_ts and not pen_ts:
        t_lo = eot
    stamps = [int(i) for i in g if i >= beg]
    if stamps:
        t = stamps[-1] - beg
        s_lo = max(s_lo, beg + (t if (last_ts and not pen_ts) else t + 1))
    if n == 0:
        t_lo, t_hi = 1, 0
        if max_initial >= 0:
            s_hi = min(s_hi, beg + max_initial)
    return t_lo, t_hi, s_lo, s_hi


def denominator(z, g=None, eot=0, beg=0, max_initial=50, timestamps=False):
    """(logsumexp of the allowed set, |L - M| of rule 5 or inf): the set the step behind g chooses from."""
    z = np.asarray(z, np.float32)
    if not timestamps:
        return logsumexp64(z), math.inf
    t_lo, t_hi, s_lo, s_hi = intervals(list(g), z.size, eot, beg, max_initial)
    text, stamps = z[t_lo:t_hi + 1] if t_lo <= t_hi else z[:0], z[s_lo:s_hi + 1] if s_lo <= s_hi else z[:0]
    _, info = ts_ref.step(z, list(g), eot, beg, max_initial)  # rule 5 is ts_ref's decision
    L = logsumexp64(stamps) if stamps.size else None
    M = float(text.max()) if text.size else None
    assert (L is None) == (info["L"] is None) and (M is None) == (info["M"] is None)
    assert L is None or L == info["L"] or abs(L - info["L"]) < 1e-9
    assert M is None or M == info["M"]
    if "mass" in info["fired"]:
        return L, info["gap_lm"]
    return logsumexp64(np.concatenate([text, stamps])), info["gap_lm"]


def token_logprob(z, tok, g=None, eot=0, beg=0, max_initial=50, timestamps=False):
    """(lp, denominator) of the id tok chosen on the fp32 logits z behind the generated ids g."""
    den, _ = denominator(z, g, eot, beg, max_initial, timestamps)
    if den == -math.inf:
        return -math.inf, den
    return float(np.float64(np.float32(z[tok])) - den), den


def no_speech_prob(z0, nosp):
    den = logsumexp64(z0)
    return 0.0 if den == -math.inf else float(math.exp(np.float64(np.float32(z0[nosp])) - den))


def decode(logits_fn, prompt, max_pos, eot, nosp, beg=0, timestamps=False, max_initial=50, stop_at_eot=True):
    """Greedy decoding over positions 0 .. max_pos - 1 with scores.  Returns a dict: ids (prompt + generated), lps (one
    per generated id), sum, n, avg, no_speech_prob, gap_lm (smallest |L - M|), gap_top (smallest top-two gap of a choice)."""
    ids = [int(i) for i in prompt]
    n_prompt = len(ids)
    nsp = no_speech_prob(logits_fn(ids[:1]), nosp)
    lps, gap_lm, gap_top = [], math.inf, math.inf
    while len(ids) <= max_pos:
        z = np.asarray(logits_fn(ids), np.float32)
        g = ids[n_prompt:]
        if timestamps:
            tok, info = ts_ref.step(z, g, eot, beg, max_initial)
            gap_lm, gap_top = min(gap_lm, info["gap_lm"]), min(gap_top, info["gap_top"])
        else:
            allowed = np.ones(z.size, bool)
            tok = ts_ref._argmax_last(z, allowed)
            gap_top = min(gap_top, ts_ref._top_two_gap(z, allowed))
        lps.append(token_logprob(z, tok, g, eot, beg, max_initial, timestamps)[0])
        ids.append(tok)
        if stop_at_eot and tok == eot:
            break
    s = float(np.sum(np.asarray(lps, np.float64)))
    return {"ids": ids, "lps": lps, "sum": s, "n": len(lps), "avg": s / len(lps), "no_speech_prob": nsp,
            "gap_lm": gap_lm, "gap_top": gap_top}


def should_skip(nsp, avg, no_speech_threshold=0.6, logprob_threshold=-1.0):
    return nsp > no_speech_threshold and not avg > logprob_threshold


def segment_scores(ids, lps, n_prompt, eot, beg, clip=0):
    """Mean lp over the text ids of every segment of ts_ref.segments(ids): [(segment, mean)]."""
    out = []
    for s in ts_ref.segments(ids, n_prompt, eot, beg, clip):
        v = [lps[i - n_prompt] for i in range(s[3], s[3] + s[4])]
        out.append((s, float(np.mean(np.asarray(v, np.float64)))))
    return out
