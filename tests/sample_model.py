"""Fixtures of the sampling tests (options temperature, temperature_fallback): the models and
clips of tests/scores_model.py, the seeds, temperatures and thresholds chosen on them on the CPU, and the reference rows
— tests/sample_ref.py over the CPU oracle — computed on demand and kept.  tests/test_sample_reference.py pins what they
give."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sample_ref as sr  # noqa: E402
import scores_model as sm  # noqa: E402

SEED = 1                      # the Philox key of the fixed-temperature decodes
OTHER_SEED = (7 << 32) | 5    # ... and of the replay that must follow its own seed (both key words set)
TEMPS = (200, 1000)           # thousandths
LOGITS_BAR = 1e-4             # the project's logits bar (section 15)
P_SHORT = sm.P_SHORT
# Fall-back on the timestamp model at P_SHORT positions over the schedule 0, 0.5, 1.0 (chosen on the CPU): clips 7 and 8
# are accepted at T = 0, clip 4 is kept at T = 0 by the silence exemption (avg_logprob -0.275 below the threshold, ratio
# 6.1 above its own, no_speech_prob 0.92), clip 2 is accepted at 0.5, clip 3 is kept at 0.5 by the silence exemption, and
# clips 0, 1, 5, 6 and 9 exhaust the schedule and keep their result at 1.0.
FB = {"seed": 1, "temperature": 0, "temperature_increment": 500, "logprob_threshold": -250,
      "compression_ratio_threshold": 3000, "no_speech_threshold": 600}
FB_TEMPS = sr.schedule(FB["temperature"], FB["temperature_increment"])


def logits_fn(model, enc_out):
    """Next-token logits of a prefix from the CPU oracle, one call per prefix: a sampled id is rarely the oracle's own
    greedy continuation, so nothing is decoded ahead (compare ts_model.logits_fn)."""
    memo = {}

    def fn(prefix):
        key = tuple(int(i) for i in prefix)
        if key not in memo:
            memo.clear()
            _, lg = model.decode_greedy(enc_out, list(key), max_positions=len(key), eot=sm.EOT, stop_at_eot=False,
                                        want_logits=True)
            memo[key] = np.asarray(lg[0], np.float32).copy()
        return memo[key]

    return fn


class Reference:
    """sample_ref.decode over the oracle for (mode, mel clip, Philox clip, temperature, seed, attempt, positions), each
    computed once.  A decode over fewer positions is the cut of a longer one that is already there."""

    def __init__(self, orc, paths, mels):
        self.orc, self.paths, self.mels = orc, paths, mels
        self.models, self.enc, self.rows = {}, {}, {}

    def close(self):
        for m in self.models.values():
            m.close()
        self.models = {}

    def _fn(self, mode, mel_clip):
        if mode not in self.models:
            self.models[mode] = self.orc.Model(self.paths[mode] + ".wtw")
        if (mode, mel_clip) not in self.enc:
            self.enc[(mode, mel_clip)] = self.models[mode].encode(self.mels[mode][mel_clip])
        return logits_fn(self.models[mode], self.enc[(mode, mel_clip)])

    def row(self, mode, mel_clip, clip, milli, seed, P, attempt=0, check=False):
        ts = mode == "ts"
        prompt = sm.TS_PROMPT if ts else sm.PLAIN_PROMPT
        for (k, r) in self.rows.items():
            if k[:6] == (mode, mel_clip, clip, milli, seed, attempt) and k[6] >= P:
                return r if k[6] == P else cut(r, P, len(prompt))
        r = sr.decode(self._fn(mode, mel_clip), prompt, P, sm.EOT, sm.NOSP, sr.temperature_of_milli(milli), seed, clip,
                      attempt, sm.BEG, ts, check=check)
        self.rows[(mode, mel_clip, clip, milli, seed, attempt, P)] = r
        return r

    def fallback(self, text_of, clips=None, clip_base=0, P=P_SHORT, fb=FB):
        """The fall-back loop per clip of the timestamp fixture (Philox clip = clip_base + index in `clips`)."""
        clips = list(range(self.mels["ts"].shape[0])) if clips is None else list(clips)
        temps = sr.schedule(fb["temperature"], fb["temperature_increment"])
        out = []
        for i, b in enumerate(clips):
            out.append(sr.decode_with_fallback(
                lambda attempt, T: self.row("ts", b, clip_base + i, temps[attempt], fb["seed"], P, attempt),
                lambda ids: text_of(ids, len(sm.TS_PROMPT)), temps, fb["compression_ratio_threshold"] / 1000.0,
                fb["logprob_threshold"] / 1000.0, fb["no_speech_threshold"] / 1000.0))
        return out


def cut(r, max_pos, n_prompt):
    """The row of a decode over max_pos positions from that of a longer one: a step depends on its prefix and on its
    position alone."""
    ids, k = r["ids"][: max_pos + 1], max_pos + 1 - n_prompt
    lps, infos = r["lps"][:k], r["infos"][:k]
    s = float(np.sum(np.asarray(lps, np.float64)))
    return dict(r, ids=ids, lps=lps, infos=infos, sum=s, n=len(lps), avg=s / len(lps))


def extra_bar(milli):
    """What the logits' error adds to a step's key bar: both keys move by at most LOGITS_BAR / T; rule 5's L and M by
    LOGITS_BAR each (T = 0: the keys are the logits)."""
    return 2.0 * LOGITS_BAR * (1000.0 / milli if milli else 1.0)


def compared_steps(r, milli):
    """Generated ids of a row that the engine must reproduce: all of them, or those before its first indecisive step."""
    s = sr.first_indecisive(r["infos"], extra_bar(milli))
    return r["n"] if s is None else s


def text_of_vocab(vocab):
    """ids -> the bytes the compression ratio is taken over (the generated ids below EOT, special tokens omitted)."""
    def f(ids, n_prompt):
        return vocab.decode(np.array([i for i in ids[n_prompt:] if i < sm.EOT], np.int64), True)
    return f
