"""Fixtures of the logit-suppression tests (wt_engine_set_suppress): the models and clips of the
tests the feature composes with (full_model, scores_model / ts_model, sample_model) and the rule that builds the lists
from the UNSUPPRESSED oracle decode, so that the filter decides something on every clip:
  always-list   per clip its most frequent generated text id (below EOT; the smallest id among equally frequent ones),
                plus ids 0 and V - 1 where they are not EOT;
  first-list    every clip's unsuppressed first generated id, plus EOT where the model's vocabulary holds it.
tests/test_suppress_reference.py pins what the lists give on the CPU; tests/test_gpu_suppress.py runs the engine against
the same rows."""
from __future__ import annotations

import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_full_ref  # noqa: E402
import full_model as fm  # noqa: E402
import scores_model as sm  # noqa: E402
import scores_ref  # noqa: E402
import suppress_ref as sup  # noqa: E402
import ts_model  # noqa: E402

P_GREEDY = fm.N_TEXT_CTX      # plain greedy: 160 positions, five 32-position segments
P_TS = sm.P_LONG              # timestamps + scores: 96
P_SHORT = sm.P_SHORT          # sampling, contexts, beam: 40, the cap inside the second segment
ASIDE_CAP = 6                 # clips set aside as indecisive: at most one in six per case
DELTA = 2e-4                  # beam sums apart by more than this (section 23)


def lists_from(rows, n_prompt, V, eot):
    """(always-list, first-list) from the unsuppressed rows (ids = prompt + generated) of a case."""
    always, first = set(), set()
    for ids in rows:
        gen = [int(i) for i in ids[n_prompt:]]
        text = [i for i in gen if i < eot]
        if text:
            c = Counter(text)
            top = max(c.values())
            always.add(min(i for i, k in c.items() if k == top))
        first.add(gen[0])
    always |= {i for i in (0, V - 1) if i != eot}
    if eot < V:
        first.add(eot)
    always.discard(eot)
    return sorted(always), sorted(first)


def check_rows(rows, plain_rows, n_prompt, always, first):
    """The pins every case must hold: the suppressed decode differs from the unsuppressed one, holds no listed id, and no
    first-list id at the first generated position."""
    for ids, plain in zip(rows, plain_rows):
        gen = [int(i) for i in ids[n_prompt:]]
        assert list(ids) != list(plain)
        assert not set(gen) & set(always)
        assert gen[0] not in set(first)


# ---- the models -------------------------------------------------------------------------------------------------------
PREV = 50361          # <|startofprev|> of the multilingual vocabulary
CONTEXT_IDS = 18      # behind this many context ids the unfiltered plain model opens some clips with <|nospeech|> itself
P_CTX = 64            # positions of the context cases: 24 fed, 40 generated


def write_eot_first(src_wtw, dst_wtw):
    """scores_model's plain model with the EOT embedding row negated: where the model's EOT logit was far below the text,
    it now is far above, and several clips open with EOT — the window Whisper's SuppressBlank exists for."""
    from wtw import read_wtw, write_wtw
    sm.write_plain_model(src_wtw, dst_wtw)
    dims, t = read_wtw(dst_wtw)
    t = {k: np.array(v) for k, v in t.items()}
    t["decoder.token_embedding.weight"][sm.EOT] *= np.float32(-1.0)
    write_wtw(dst_wtw, dims, t)


def context(n, seed=0):
    rng = np.random.default_rng(100 + n + 1000 * seed)
    return [int(i) for i in rng.integers(0, sm.EOT, size=n)]


def fed(ctx, prompt):
    return ([PREV] + list(ctx) if len(ctx) else []) + list(prompt)


def decode_row(raw_fn, fed_prompt, n_tail, max_pos, timestamps, always=(), first=(), milli=0, seed=0, clip=0, attempt=0,
               nosp=sm.NOSP):
    """One clip behind the filter, in the style of scores_ref.decode: sample_ref.decode (T = 0: the greedy step) over the
    wrapped logits function; no_speech_prob from the UNFILTERED logits behind sot (nosp: the id, any id of a vocabulary
    without one); first = the first indecisive step at the bar sample_model.extra_bar gives (None: the clip is decisive)."""
    import sample_model
    import sample_ref
    n0 = len(fed_prompt)
    fn = sup.wrap(raw_fn, n0, always, first)
    r = sample_ref.decode(fn, fed_prompt, max_pos, sm.EOT, nosp, sample_ref.temperature_of_milli(milli), seed, clip, attempt,
                          sm.BEG, timestamps)
    r["no_speech_prob"] = scores_ref.no_speech_prob(raw_fn(fed_prompt[: n0 - n_tail + 1]), nosp)
    r["first"] = sample_ref.first_indecisive(r["infos"], sample_model.extra_bar(milli))
    r["n0"] = n0
    return r


def other_lists(lists, row, n_prompt):
    """Lists of the same counts and other contents: the always-list's second id gives way to the most frequent text id
    the SUPPRESSED row generated, so that the decode behind them differs again."""
    c = Counter(i for i in row["ids"][n_prompt:] if i < sm.EOT and i not in lists[0])
    top = max(c.values())
    alt = min(i for i, k in c.items() if k == top)
    return sorted([i for i in lists[0] if i != lists[0][1]] + [alt]), list(lists[1])


def compared(r):
    """Ids of a row the engine must reproduce: all of them, or those before the first indecisive step."""
    return r["ids"] if r["first"] is None else r["ids"][: r["n0"] + r["first"]]


TS_CLIPS, FIRST_CLIPS, RICH_CLIPS, DENSE_CLIPS = (0, 1, 2), tuple(range(12)), tuple(range(6)), (0, 1)
P_DENSE = 64


def write_models(prefix, vocab, d):
    """The four models of the suppression tests under directory d: name -> (model prefix, vocabulary file)."""
    paths = {k: os.path.join(d, "micro-sup-" + k) for k in ("ts", "first", "rich", "dense")}
    sm.write_ts_model(prefix + ".wtw", paths["ts"] + ".wtw")
    write_eot_first(prefix + ".wtw", paths["first"] + ".wtw")
    fm.write_eot_rich(prefix + ".wtw", paths["rich"] + ".wtw")
    fm.write_dense(prefix + ".wtw", paths["dense"] + ".wtw")
    return {k: (v, vocab) for k, v in paths.items()}


def all_mels():
    out = {"ts": sm.ts_mels(), "first": sm.plain_mels(), "rich": sm.plain_mels(), "dense": fm.dense_mels((80, 200))}
    for m in out.values():
        m.setflags(write=False)
    return out


class Reference:
    """Rows of suppress_model.decode_row over the oracle, each computed once on demand and never changed."""

    def __init__(self, orc, models, mels):
        self.orc, self.paths, self.mels = orc, models, mels
        self.models, self.enc, self.rows, self.lists = {}, {}, {}, {}

    def close(self):
        for m in self.models.values():
            m.close()

    def raw(self, mode, clip, max_pos, lookahead=True):
        if mode not in self.models:
            self.models[mode] = self.orc.Model(self.paths[mode][0] + ".wtw")
        if (mode, clip) not in self.enc:
            self.enc[(mode, clip)] = self.models[mode].encode(self.mels[mode][clip])
        if lookahead:
            return ts_model.logits_fn(self.models[mode], self.enc[(mode, clip)], max_pos)
        return beam_full_ref.level_logits_fn(self.models[mode], self.enc[(mode, clip)], sm.EOT)

    def row(self, mode, clip, max_pos, lists=((), ()), ctx=(), milli=0, seed=0, rng_clip=0, attempt=0, prompt=None):
        key = (mode, clip, max_pos, tuple(lists[0]), tuple(lists[1]), tuple(ctx), milli, seed, rng_clip, attempt)
        if key not in self.rows:
            ts = mode == "ts"
            tail = list(prompt if prompt is not None else (sm.TS_PROMPT if ts else sm.PLAIN_PROMPT))
            self.rows[key] = decode_row(self.raw(mode, clip, max_pos), fed(ctx, tail), len(tail), max_pos, ts,
                                            lists[0], lists[1], milli, seed, rng_clip, attempt,
                                            nosp=0 if mode == "dense" else sm.NOSP)
        return self.rows[key]

    def lists_of(self, mode, clips, max_pos, prompt=None, V=ts_model.N_VOCAB):
        key = (mode, tuple(clips), max_pos)
        if key not in self.lists:
            plain = [self.row(mode, b, max_pos, prompt=prompt)["ids"] for b in clips]
            n0 = len(prompt) if prompt is not None else (len(sm.TS_PROMPT if mode == "ts" else sm.PLAIN_PROMPT))
            self.lists[key] = lists_from(plain, n0, V, sm.EOT)
        return self.lists[key]
