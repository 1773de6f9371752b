"""Reference timestamp decoding: the rules of DESIGN.md section 14 (option timestamps) and the segment parser, restated
in Python over any next-token logits function — the CPU oracle (beam_ref.oracle_logits_fn) for the parity tests,
hand-made tables for the rule tests.

With g the ids generated so far, tick(id) = id - beg, last_ts = g[-1] >= beg, pen_ts = |g| < 2 or g[-2] >= beg:
  1. eot < id < beg is masked;
  2. last_ts and pen_ts: id >= beg masked; last_ts and not pen_ts: id < eot masked;
  3. t = tick of the last timestamp in g: ticks below t (last_ts and not pen_ts) or below t + 1 (otherwise) masked;
  4. |g| = 0: id < beg masked, and ticks above max_initial when that is >= 0;
  5. L = logsumexp of the unmasked logits with id >= beg (float64 from the fp32 logits), M = the largest unmasked logit
     with id < beg; both exist and L > M: id < beg masked;
  6. argmax of what is left: larger logit, then larger id; -0 and +0 are one value."""
from __future__ import annotations

import math

import numpy as np

WINDOW_MS = 30000
RULES = ("text_after_pair", "text_forbidden", "monotonic", "initial", "mass")


def _argmax_last(z, allowed):
    """Largest allowed logit, the larger id on equal logits (-0 == +0 in numpy too)."""
    idx = np.flatnonzero(allowed)
    v = z[idx]
    return int(idx[np.flatnonzero(v == v.max())[-1]])


def _top_two_gap(z, allowed):
    v = np.sort(z[allowed].astype(np.float64))
    if v.size < 2:
        return math.inf
    return 0.0 if v[-1] == v[-2] else float(v[-1] - v[-2])


def step(z, g, eot, beg, max_initial=50):
    """One filtered greedy step on the fp32 logits z behind the generated ids g.  Returns (token, info): info holds L, M
    (None where no such id is allowed), gap_lm = |L - M| (inf where rule 5 has nothing to decide), gap_top = the top-two
    gap of the final argmax, fired = the rules that masked an id which would otherwise have been allowed, and
    plain = the argmax of the unfiltered logits."""
    z = np.asarray(z, np.float32)
    V = z.size
    ids = np.arange(V)
    fired = set()
    allowed = ~((ids > eot) & (ids < beg))                                   # rule 1
    n = len(g)
    last_ts = n >= 1 and g[-1] >= beg
    pen_ts = n < 2 or g[-2] >= beg
    if last_ts and pen_ts:                                                   # rule 2
        allowed &= ids < beg
        fired.add("text_after_pair")
    if last_ts and not pen_ts:
        allowed &= ids >= eot
        fired.add("text_forbidden")
    stamps = [int(i) for i in g if i >= beg]
    if stamps:                                                               # rule 3
        t = stamps[-1] - beg
        lo = beg + (t if (last_ts and not pen_ts) else t + 1)
        before = allowed.copy()
        allowed &= ~((ids >= beg) & (ids < lo))
        if (before != allowed).any():
            fired.add("monotonic")
            # the id that would have won without this rule
            if _argmax_last(z, before) != _argmax_last(z, allowed) and before[beg:].any():
                fired.add("monotonic_decided")
    if n == 0:                                                               # rule 4
        allowed &= ids >= beg
        if max_initial >= 0:
            allowed &= ids <= beg + max_initial
        fired.add("initial")
    ts_ok, tx_ok = allowed & (ids >= beg), allowed & (ids < beg)
    L = M = None
    gap_lm = math.inf
    if ts_ok.any():
        zs = z[ts_ok].astype(np.float64)
        m = zs.max()
        L = float(m + math.log(np.exp(zs - m).sum())) if m != -math.inf else -math.inf
    if tx_ok.any():
        M = float(z[tx_ok].max())
    if L is not None and M is not None:                                      # rule 5
        gap_lm = 0.0 if L == M else abs(L - M)
        if L > M:
            allowed = ts_ok
            fired.add("mass")
            if float(z[ts_ok].max()) <= M:
                fired.add("mass_decided")  # no single timestamp logit exceeds M: a plain masked argmax picks text
    tok = _argmax_last(z, allowed)                                           # rule 6
    info = {"L": L, "M": M, "gap_lm": gap_lm, "gap_top": _top_two_gap(z, allowed), "fired": fired,
            "plain": _argmax_last(z, np.ones(V, bool))}
    return tok, info


def decode(logits_fn, prompt, max_pos, eot, beg, max_initial=50, stop_at_eot=True):
    """Filtered greedy decoding over positions 0 .. max_pos - 1 (the oracle's max_positions): returns (ids = prompt +
    generated, infos = step()'s info per generated id)."""
    ids = [int(i) for i in prompt]
    n_prompt = len(ids)
    infos = []
    while len(ids) <= max_pos:
        tok, info = step(logits_fn(ids), ids[n_prompt:], eot, beg, max_initial)
        ids.append(tok)
        infos.append(info)
        if stop_at_eot and tok == eot:
            break
    return ids, infos


def first_indecisive(infos, bar):
    """Index of the first step either of whose decision gaps is at or below `bar` (None: the clip is decisive)."""
    for s, info in enumerate(infos):
        if info["gap_lm"] <= bar or info["gap_top"] <= bar:
            return s
    return None


def segments(ids, sample_begin, eot, beg, clip=0):
    """The segment parser of DESIGN.md section 14: tuples (clip, t0_ms, t1_ms, id_begin, id_count, open)."""
    out = []
    t_open, begin, count = 0, -1, 0
    for i in range(sample_begin, len(ids)):
        tok = int(ids[i])
        if tok == eot:
            break
        if tok >= beg:
            ms = min(tok - beg, 1500) * 20
            if count > 0:
                out.append((clip, t_open, ms, begin, count, 0))
            t_open, begin, count = ms, -1, 0
        else:
            if count == 0:
                begin = i
            count += 1
    if count > 0:
        out.append((clip, t_open, WINDOW_MS, begin, count, 1))
    return out
