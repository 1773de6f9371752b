"""Reference seeking transcription: the loop of DESIGN.md section 20 (options seek, condition_on_previous_text and the
context of wt_engine_set_context) restated in Python over any per-window decode function, and such a function over any
next-token logits function — the CPU oracle for the parity tests, hand-made rows for the rule tests.

A tick is 320 samples = 20 ms.  With g the ids a window generated before its first EOT, ts(i) = g[i] >= beg and
tick(id) = min(max(id - beg, 0), win_ticks):
  single_end = n >= 2 and ts(n - 1) and not ts(n - 2);  cons = [i >= 1 : ts(i - 1) and ts(i)]
  cons not empty: the row is cut at every i of cons, and at n when single_end; a slice g[last:cur] is a segment from
      tick(g[last]) to tick(g[cur - 1]); advance = seg_ticks when single_end, else tick(g[last cut - 1]); ids behind the
      last cut are dropped (the next window decodes them again)
  cons empty: one segment holding all of g, from 0 to the last timestamp's tick when there is one and it is not tick 0,
      else to seg_ticks with open = 1; advance = seg_ticks
  a segment with no id below eot, or with t0 == t1, is dropped; advance == 0 becomes seg_ticks."""
from __future__ import annotations

import math

import numpy as np

import scores_ref
import ts_ref

TICK = 320  # samples


def seek_step(g, eot, beg, win_ticks, seg_ticks):
    """(segments, advance): segments are tuples (0, t0_ms, t1_ms, id_begin, id_count, open) with g[id_begin : id_begin +
    id_count] the slice, timestamps included; branch() names the path taken."""
    g = [int(i) for i in g]
    n = len(g)
    ts = [i >= beg for i in g]

    def tick(i):
        return min(max(i - beg, 0), win_ticks)

    segs = []

    def push(first, end, t0, t1, is_open):
        if any(i < eot for i in g[first:end]) and t0 != t1:
            segs.append((0, t0 * 20, t1 * 20, first, end - first, is_open))

    single_end = n >= 2 and ts[-1] and not ts[-2]
    cons = [i for i in range(1, n) if ts[i - 1] and ts[i]]
    if cons:
        cuts = cons + ([n] if single_end else [])
        last = 0
        for cur in cuts:
            push(last, cur, tick(g[last]), tick(g[cur - 1]), 0)
            last = cur
        advance = seg_ticks if single_end else tick(g[last - 1])
    else:
        stamps = [i for i in g if i >= beg]
        if stamps and stamps[-1] != beg:
            push(0, n, 0, tick(stamps[-1]), 0)
        else:
            push(0, n, 0, seg_ticks, 1)
        advance = seg_ticks
    if advance == 0:
        advance = seg_ticks
    return segs, advance


def branch(g, beg):
    """Which path of seek_step a row takes: 'pairs', 'pairs_single_end', 'no_pair_stamp' (a trailing timestamp other than
    tick 0 ends the one segment) or 'no_pair_open'."""
    g = [int(i) for i in g]
    ts = [i >= beg for i in g]
    n = len(g)
    if any(ts[i - 1] and ts[i] for i in range(1, n)):
        return "pairs_single_end" if n >= 2 and ts[-1] and not ts[-2] else "pairs"
    stamps = [i for i in g if i >= beg]
    return "no_pair_stamp" if stamps and stamps[-1] != beg else "no_pair_open"


def fed_prompt(context, prompt, prev, keep):
    """[prev] + the last `keep` ids of the context + prompt; the prompt alone without a context."""
    context = [int(i) for i in context]
    if not context or keep < 1:
        return [int(i) for i in prompt]
    return [int(prev)] + context[-keep:] + [int(i) for i in prompt]


def transcribe(decode_window, n_samples, win, eot, beg, prev, prompt, keep, context=(), condition=True):
    """The loop.  decode_window(w, seek, fed) decodes the window that starts at sample `seek` behind the prompt `fed`
    and returns a dict with at least ids (fed + generated) and optionally skipped, temperature_milli and whatever else
    the caller wants kept.  Returns one dict per window: that dict plus seek, advance (samples), n_context, n_prompt,
    gen (g), segments (in the file's time, id_begin an index into ids), kept (ids) and branch."""
    win_ticks = win // TICK
    ctx = [int(i) for i in context]
    seek, w, out = 0, 0, []
    while True:
        seg_ticks = min(win_ticks, max(0, -(-(n_samples - seek) // TICK)))
        fed = fed_prompt(ctx, prompt, prev, keep)
        r = dict(decode_window(w, seek, fed))
        ids = [int(i) for i in r["ids"]]
        assert ids[: len(fed)] == fed
        g = ids[len(fed):]
        if eot in g:
            g = g[: g.index(eot)]
        kept, segs, advance, path = [], [], seg_ticks, "skipped"
        if not r.get("skipped", False):
            raw, advance = seek_step(g, eot, beg, win_ticks, seg_ticks)
            path = branch(g, beg)
            for (_, t0, t1, b, c, o) in raw:
                kept += g[b:b + c]
                segs.append((w, seek // 16 + t0, seek // 16 + t1, len(fed) + b, c, o))
        n_ctx = len(fed) - len(prompt) - 1 if len(fed) > len(prompt) else 0
        r.update(seek=seek, advance=advance * TICK, n_context=n_ctx, n_prompt=len(fed), gen=g, segments=segs, kept=kept,
                 branch=path)
        out.append(r)
        ctx += kept
        if not r.get("skipped", False) and (not condition or r.get("temperature_milli", 0) > 500):
            ctx = []
        seek += advance * TICK
        w += 1
        if seek >= n_samples:
            return out


def window_decoder(logits_fn_of, n_tail, max_pos, eot, beg, nosp=None, max_initial=50, no_speech_threshold=0.6,
                   logprob_threshold=-1.0, skip_silence=False):
    """A decode_window for transcribe() over next-token logits: logits_fn_of(w, seek) -> logits_fn(prefix).  Timestamp
    decoding (ts_ref); with nosp the scores of scores_ref as well.  n_tail = the length of the prompt proper, whose first
    id is sot: the no-speech logits are those behind fed[: index(sot) + 1], index(sot) = len(fed) - n_tail."""

    def decode(w, seek, fed):
        fn = logits_fn_of(w, seek)
        n0, ids, lps, gap_lm, gap_top = len(fed), [int(i) for i in fed], [], math.inf, math.inf
        r = {}
        if nosp is not None:
            r["no_speech_prob"] = scores_ref.no_speech_prob(fn(ids[: n0 - n_tail + 1]), nosp)
        while len(ids) <= max_pos:
            z = np.asarray(fn(ids), np.float32)
            g = ids[n0:]
            tok, info = ts_ref.step(z, g, eot, beg, max_initial)
            gap_lm, gap_top = min(gap_lm, info["gap_lm"]), min(gap_top, info["gap_top"])
            if nosp is not None:
                lps.append(scores_ref.token_logprob(z, tok, g, eot, beg, max_initial, True)[0])
            ids.append(tok)
            if tok == eot:
                break
        r.update(ids=ids, gap_lm=gap_lm, gap_top=gap_top)
        if nosp is not None:
            total = float(np.sum(np.asarray(lps, np.float64)))
            r.update(lps=lps, sum=total, n=len(lps), avg=total / len(lps))
            r["skipped"] = bool(skip_silence and scores_ref.should_skip(r["no_speech_prob"], r["avg"], no_speech_threshold,
                                                                        logprob_threshold))
        return r

    return decode


def smallest_margin(windows):
    """The smallest decisive margin (top-two gap and |L - M|) over all steps of all windows."""
    return min([math.inf] + [min(r["gap_lm"], r["gap_top"]) for r in windows if "gap_lm" in r])
