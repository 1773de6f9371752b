"""Reference full-length beam search: the rules of DESIGN.md section 23 (option full_beam), restated in Python over any
next-token logits function — the CPU oracle for the fixture pins, hand-made tables for the rule tests.

The walk, the finished list, the cap fill and the ranker are section 11's (tests/beam_ref.py).  What is new: every live
hypothesis first applies the step's allowed set A to its OWN generated ids g.  Without timestamps A is the whole
vocabulary; with them A is what rules 1 to 5 of section 14 (tests/ts_ref.py) leave on g, rule 5 decided in float64 from
the fp32 logits.  A logit of -inf is a masked id whatever the rules say (that is what masking is), so it is never in A.
lp(id) = z[id] - logsumexp_A(z), in float64: filter first, then log-softmax.  A hypothesis offers its top K+1 ids of A by
logit, the larger id first on equal logits (-0 and +0 are one value); when A holds fewer it offers what A holds.  A step
whose walk finds fewer than K non-EOT candidates leaves fewer live hypotheses; a clip is done when it has K finished
hypotheses or no live one."""
from __future__ import annotations

import math

import numpy as np

import beam_ref

GAP_KINDS = beam_ref.GAP_KINDS + ("mass",)


def level_logits_fn(model, enc_out, eot):
    """Next-token logits of a prefix from the CPU oracle, memoised for a search that moves level by level: only prefixes
    within one id of the current length are kept (a row of logits is 200 KB, a search visits thousands)."""
    memo = {}

    def fn(prefix):
        key = tuple(int(i) for i in prefix)
        if key not in memo:
            for old in [k for k in memo if abs(len(k) - len(key)) > 1]:
                del memo[old]
            _, lg = model.decode_greedy(enc_out, list(key), max_positions=len(key), eot=eot, stop_at_eot=False,
                                        want_logits=True)
            memo[key] = np.asarray(lg[0], np.float32).copy()
        return memo[key]

    return fn


def allowed_set(z, g, eot, beg, max_initial=50):
    """Rules 1 to 5 of section 14 on the fp32 logits z behind the generated ids g: (A as a boolean mask, |L - M| of rule
    5 — inf where it has nothing to decide)."""
    z = np.asarray(z, np.float32)
    ids = np.arange(z.size)
    allowed = ~((ids > eot) & (ids < beg))                                   # rule 1
    n = len(g)
    last_ts = n >= 1 and g[-1] >= beg
    pen_ts = n < 2 or g[-2] >= beg
    if last_ts and pen_ts:                                                   # rule 2
        allowed &= ids < beg
    if last_ts and not pen_ts:
        allowed &= ids >= eot
    stamps = [int(i) for i in g if i >= beg]
    if stamps:                                                               # rule 3
        t = stamps[-1] - beg
        allowed &= ~((ids >= beg) & (ids < beg + (t if (last_ts and not pen_ts) else t + 1)))
    if n == 0:                                                               # rule 4
        allowed &= ids >= beg
        if max_initial >= 0:
            allowed &= ids <= beg + max_initial
    allowed &= z != -np.inf
    ts_ok, tx_ok = allowed & (ids >= beg), allowed & (ids < beg)
    gap_lm = math.inf
    if ts_ok.any() and tx_ok.any():                                          # rule 5
        zs = z[ts_ok].astype(np.float64)
        m = zs.max()
        L = float(m + math.log(np.exp(zs - m).sum()))
        M = float(z[tx_ok].max())
        gap_lm = 0.0 if L == M else abs(L - M)
        if L > M:
            allowed = ts_ok
    return allowed, gap_lm


def step_lp(z, g, eot, beg=None, timestamps=False, max_initial=50):
    """(lp [V] float64 with -inf outside A, |L - M|) of one hypothesis."""
    z = np.asarray(z, np.float32)
    if timestamps:
        allowed, gap_lm = allowed_set(z, g, eot, beg, max_initial)
    else:
        allowed, gap_lm = z != -np.inf, math.inf
    lp = np.full(z.size, -np.inf)
    if allowed.any():
        za = z[allowed].astype(np.float64)
        m = za.max()
        lp[allowed] = za - (m + math.log(np.exp(za - m).sum()))
    return lp, gap_lm


def offered(lp, K):
    """The ids a hypothesis offers: the top K+1 of A (lp > -inf) by lp — within one hypothesis that is the order of the
    logits — larger id first on equal values; then the K+2nd for the cut gap, where A holds one."""
    order = beam_ref.ranked(lp, K + 2)
    return [int(i) for i in order if lp[i] != -np.inf]


def _result(prompt, K, live, finished, margin, gaps, done, eot_slots, n_live):
    """The cap fill and the ranker of section 11 on copies of a search's state."""
    n_prompt = len(prompt)
    finished = list(finished)
    gaps = {k: list(v) for k, v in gaps.items()}
    if not done:
        for seq, sm, lps in live:
            if len(finished) >= K:
                break
            finished.append((seq[n_prompt:], sm, lps))
    norm = [sm / len(gen) for gen, sm, _ in finished]
    best = 0
    for i, v in enumerate(norm):
        if v > norm[best]:
            best = i
    if len(norm) > 1:
        rest = sorted(norm, reverse=True)
        margin = min(margin, rest[0] - rest[1])
    gaps["final"] += [beam_ref._gap(norm[best], v) for i, v in enumerate(norm) if i != best]
    gen, sm, lps = finished[best] if finished else ([], 0.0, [])
    return {"ids": prompt + gen, "lps": lps, "sum": sm, "n_gen": len(gen), "margin": margin, "done_early": done,
            "eot_slots": list(eot_slots), "gaps": gaps, "n_live": list(n_live), "finished": [(g, s) for g, s, _ in finished]}


def beam_search(logits_fn, prompt, K, max_pos, eot, beg=None, timestamps=False, max_initial=50):
    """Returns dict(ids, lps, sum, n_gen, margin, done_early, eot_slots, gaps, n_live, finished): ids = prompt + generated
    (EOT included), lps = the log-probabilities of the generated ids under A; margin = the smallest decision gap met,
    gaps = every gap by kind (beam_ref.GAP_KINDS and "mass", rule 5's |L - M| of every live hypothesis); n_live = live
    hypotheses entering each step; finished = the finished list (generated ids, sum) in the order it was filled.
    max_pos may be a tuple of caps: every step depends on its prefixes alone, so the search to a shorter cap is the longer
    one stopped there; the result is then a dict of results by cap."""
    caps = (max_pos,) if isinstance(max_pos, int) else tuple(max_pos)
    prompt = [int(i) for i in prompt]
    n_prompt = len(prompt)
    live = [(prompt, 0.0, [])]
    finished = []  # (generated ids incl. EOT, sum, lps)
    margin = math.inf
    eot_slots, n_live = [], []
    gaps = {k: [] for k in GAP_KINDS}
    done = False
    out = {}
    for step in range(max(caps) - n_prompt + 1):
        n_live.append(len(live))
        cands = []
        for s, (seq, sm, lps) in enumerate(live):
            lp, gap_lm = step_lp(logits_fn(seq), seq[n_prompt:], eot, beg, timestamps, max_initial)
            if gap_lm != math.inf:
                gaps["mass"].append(gap_lm)
                margin = min(margin, gap_lm)
            order = offered(lp, K)
            gaps["logit"] += [beam_ref._gap(lp[order[r]], lp[order[r + 1]]) for r in range(min(K, len(order) - 1))]
            if len(order) > K + 1:
                g = beam_ref._gap(lp[order[K]], lp[order[K + 1]])
                gaps["cut"].append(g)
                margin = min(margin, g)
            for r in range(min(K + 1, len(order))):
                tok = order[r]
                cands.append((sm + lp[tok], s, r, tok, seq, lps + [float(lp[tok])]))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        new_live = []
        walked = len(cands)
        for i, (sc, s, _r, tok, seq, lps) in enumerate(cands):
            if tok == eot:
                if len(finished) < K:
                    finished.append((seq[n_prompt:] + [tok], sc, lps))
                    eot_slots.append(s)
            else:
                new_live.append((seq + [tok], sc, lps))
                if len(new_live) == K:
                    if i + 1 < len(cands):
                        margin = min(margin, sc - cands[i + 1][0])
                    walked = i + 1
                    break
        gaps["score"] += [beam_ref._gap(cands[i][0], cands[i + 1][0]) for i in range(min(walked, len(cands) - 1))
                          if cands[i][1] != cands[i + 1][1]]
        live = new_live
        done = len(finished) >= K
        ended = done or not live
        for cap in caps:  # the caps whose last step this was, and at the end of the search every longer one
            if cap not in out and (ended or cap - n_prompt == step):
                out[cap] = _result(prompt, K, live, finished, margin, gaps, done, eot_slots, n_live)
        if ended:
            break
    return out[caps[0]] if isinstance(max_pos, int) else out


def teacher_forced(logits_fn, ids, n_prompt, eot, beg=None, timestamps=False, max_initial=50):
    """The log-probabilities (float64) of ids[n_prompt:] under A given their prefixes, and their sum."""
    lps = [float(step_lp(logits_fn(ids[:i]), ids[n_prompt:i], eot, beg, timestamps, max_initial)[0][int(ids[i])])
           for i in range(n_prompt, len(ids))]
    return lps, math.fsum(lps)
