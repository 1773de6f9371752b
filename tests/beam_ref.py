"""Reference beam search: the rules of DESIGN.md section 11 (option beam_size), restated in Python over any
next-token logits function — the CPU oracle for the parity tests, hand-made tables for the rule tests.

lp = z - logsumexp(z) in float64 from the fp32 logits z of a hypothesis; its top K+1 tokens by lp (equal lp: the
larger id first); candidates (slot s, rank r, token, sum_s + lp[token]) ordered by score, then lower s, then lower r;
the walk appends EOT candidates to the finished list while it holds fewer than K and makes every other candidate the
next live hypothesis until K exist; a clip with K finished hypotheses is done; after the last step the live
hypotheses fill the finished list in slot order; the result is the first best sum / n_gen (EOT counted)."""
from __future__ import annotations

import math

import numpy as np


def oracle_logits_fn(model, enc_out, eot):
    """Next-token logits of a prefix from the CPU oracle (memoised: hypotheses of several beam sizes share prefixes)."""
    memo = {}

    def fn(prefix):
        key = tuple(int(i) for i in prefix)
        if key not in memo:
            _, lg = model.decode_greedy(enc_out, list(key), max_positions=len(key), eot=eot, stop_at_eot=False,
                                        want_logits=True)
            memo[key] = np.asarray(lg[0], np.float32).copy()
        return memo[key]

    return fn


def log_softmax64(z):
    z = np.asarray(z, np.float32).astype(np.float64)
    m = z.max()
    return z - (m + math.log(np.exp(z - m).sum()))


def ranked(lp, n=None):
    """Token ids by lp descending, equal lp: larger id first (-0 and +0 are one value, -inf entries come last); n: only
    the first n of that order (every entry tied with the n-th is sorted, so the prefix is the same)."""
    lp = np.asarray(lp)
    ids = np.arange(lp.size)
    if n is not None and n < lp.size:
        cut = np.partition(lp, lp.size - n)[lp.size - n]  # the n-th largest value
        ids = np.flatnonzero(lp >= cut)
        return ids[np.lexsort((-ids, -lp[ids]))][:n]
    return np.lexsort((-ids, -lp))


def _gap(a, b):
    """a - b of two ordered values; 0 when they are equal (also two -inf)."""
    return 0.0 if a == b else float(a - b)


GAP_KINDS = ("logit", "cut", "score", "final")


def beam_search(logits_fn, prompt, K, max_pos, eot):
    """Returns dict(ids, sum, n_gen, margin, done_early, eot_slots, gaps, eot_dropped): ids = prompt + generated (EOT
    included); margin = the smallest decision gap met (rank K+1 / K+2 of every hypothesis, last candidate taken / first
    not taken of every walk, best / second-best final normalised score); done_early = K finished before the last step;
    eot_slots = slots the accepted EOT candidates came from; gaps = every decision gap by kind (GAP_KINDS; 0 = a tie the
    rules decide): "logit" adjacent lp among a hypothesis's top K+1, "cut" its ranks K+1 / K+2, "score" adjacent
    candidates of different slots in the walked part of a step's order (the first one not walked included), "final"
    the first best normalised score against every other entry; eot_dropped = EOT candidates walked past a full list."""
    prompt = [int(i) for i in prompt]
    n_prompt = len(prompt)
    n_steps = max_pos - n_prompt + 1
    live = [(prompt, 0.0)]
    finished = []  # (generated ids incl. EOT, sum)
    margin = math.inf
    eot_slots = []
    gaps = {k: [] for k in GAP_KINDS}
    eot_dropped = 0
    done = False
    for _ in range(n_steps):
        cands = []
        for s, (seq, sm) in enumerate(live):
            lp = log_softmax64(logits_fn(seq))
            order = ranked(lp, K + 2)
            gaps["logit"] += [_gap(lp[order[r]], lp[order[r + 1]]) for r in range(min(K, order.size - 1))]
            if order.size > K + 1:
                g = _gap(lp[order[K]], lp[order[K + 1]])
                gaps["cut"].append(g)
                margin = min(margin, g)
            for r in range(min(K + 1, order.size)):
                tok = int(order[r])
                cands.append((sm + lp[tok], s, r, tok, seq))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        new_live = []
        walked = len(cands)
        for i, (sc, s, _r, tok, seq) in enumerate(cands):
            if tok == eot:
                if len(finished) < K:
                    finished.append((seq[n_prompt:] + [tok], sc))
                    eot_slots.append(s)
                else:
                    eot_dropped += 1
            else:
                new_live.append((seq + [tok], sc))
                if len(new_live) == K:
                    if i + 1 < len(cands):
                        margin = min(margin, sc - cands[i + 1][0])
                    walked = i + 1
                    break
        gaps["score"] += [_gap(cands[i][0], cands[i + 1][0]) for i in range(min(walked, len(cands) - 1))
                          if cands[i][1] != cands[i + 1][1]]
        live = new_live
        if len(finished) >= K:
            done = True
            break
    if not done:
        for seq, sm in live:
            if len(finished) >= K:
                break
            finished.append((seq[n_prompt:], sm))
    norm = [sm / len(gen) for gen, sm in finished]
    best = 0
    for i, v in enumerate(norm):
        if v > norm[best]:
            best = i
    if len(norm) > 1:
        rest = sorted(norm, reverse=True)
        margin = min(margin, rest[0] - rest[1])
    gaps["final"] += [_gap(norm[best], v) for i, v in enumerate(norm) if i != best]
    gen, sm = finished[best]
    return {"ids": prompt + gen, "sum": sm, "n_gen": len(gen), "margin": margin, "done_early": done,
            "eot_slots": eot_slots, "gaps": gaps, "eot_dropped": eot_dropped}


def teacher_forced_sum(logits_fn, ids, n_prompt):
    """Sum of log-probabilities (float64) of ids[n_prompt:] given their prefixes."""
    total = 0.0
    for i in range(n_prompt, len(ids)):
        total += log_softmax64(logits_fn(ids[:i]))[int(ids[i])]
    return total
