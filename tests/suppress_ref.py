"""Reference logit suppression (wt_engine_set_suppress): Whisper's SuppressTokens and SuppressBlank
as a function on a row of logits, composed in FRONT of the references the project already has, and a restatement of the
default lists wt_vocab_default_suppress builds.

The filter: the listed ids get -inf, the first-list only where nothing has been generated yet (n_gen == 0, the position
behind the whole fed prompt and context).  Every other reference (ts_ref, scores_ref, sample_ref, beam_full_ref) takes a
next-token logits function of a prefix; `wrap` puts the filter on such a function, so the rules, the log-softmax, the
sampler and every beam hypothesis see a vocabulary without the listed ids.  A prefix shorter than the prompt is not a
generated position and stays as it is: the no-speech probability is read there, from the unfiltered logits."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ts_ref  # noqa: E402

# Whisper's non_speech_tokens, typed out: single characters, then the multi-character marks, then the musical symbols
SYMBOLS = list("\"#()*+/:;<=>@[\\]^_`{|}~「」『』") + (
    "<< >> <<< >>> -- --- -( -[ (' (\" (( )) ((( ))) [[ ]] {{ }} ♪♪ ♪♪♪".split())
MUSICAL = list("♩♪♫♬♭♮♯")


def filter_row(z, n_gen, ids=(), first_ids=()):
    """The filtered copy of the fp32 logits z of a clip that has generated n_gen ids."""
    z = np.array(z, np.float32, copy=True)
    if len(ids):
        z[np.asarray(ids, np.int64)] = -np.inf
    if n_gen == 0 and len(first_ids):
        z[np.asarray(first_ids, np.int64)] = -np.inf
    return z


def wrap(logits_fn, n_prompt, ids=(), first_ids=()):
    """logits_fn(prefix) with the filter in front; n_prompt = the fed prompt's length, context included."""
    def fn(prefix):
        z = logits_fn(prefix)
        n_gen = len(prefix) - n_prompt
        return z if n_gen < 0 else filter_row(z, n_gen, ids, first_ids)
    return fn


def greedy(logits_fn, prompt, max_pos, eot, ids=(), first_ids=(), stop_at_eot=True):
    """Plain greedy decoding behind the filter, the loop of full_model.oracle_rows: returns (ids = prompt + generated,
    margins = the top-two gap over the allowed set of every step; larger logit, then larger id)."""
    fn = wrap(logits_fn, len(prompt), ids, first_ids)
    row = [int(i) for i in prompt]
    margins = []
    while len(row) <= max_pos:
        z = fn(row)
        allowed = z > -np.inf
        assert allowed.any()
        tok = ts_ref._argmax_last(z, allowed)
        margins.append(ts_ref._top_two_gap(z, allowed))
        row.append(tok)
        if stop_at_eot and tok == eot:
            break
    return row, np.asarray(margins, np.float64)


def default_lists(tokens, info, n_limit=None):
    """wt_vocab_default_suppress restated: tokens = {id: bytes} of the vocabulary, info = its special ids (Vocab.info()),
    n_limit = ids below it only (default info["n_vocab"]).  Returns (ids, first_ids), sorted and unique."""
    n_limit = info["n_vocab"] if n_limit is None else n_limit
    text_end = min(n_limit, info["eot"])
    by_bytes = {}
    for i in sorted(tokens):
        if 0 <= i < text_end:
            by_bytes.setdefault(bytes(tokens[i]), i)  # the smallest id of equal bytes

    def exact(s):
        return by_bytes.get(s.encode("utf-8"), -1)

    def prefix(s, above):
        s = s.encode("utf-8")
        best, length = -1, above
        for i in sorted(tokens):
            t = bytes(tokens[i])
            if 0 <= i < text_end and t and len(t) < len(s) and s.startswith(t) and len(t) > length:
                best, length = i, len(t)
        return best

    # <|startoflm|> is the id in front of <|startofprev|>; the table's "solm" is the <|nospeech|> id
    special = [info[k] for k in ("sot", "prev", "solm", "translate", "transcribe")] + [info["prev"] - 1]
    out = [i for i in special if 0 <= i < n_limit and i != info["eot"]]
    out += [exact(" -"), exact(" '")]
    for s in SYMBOLS:
        out += [exact(s), exact(" " + s)]
    for s in MUSICAL:
        for lead in (0, 1):
            w = (" " if lead else "") + s
            i = exact(w)
            out.append(i if i >= 0 else prefix(w, lead))  # behind the space the prefix must reach into the symbol
    first = [exact(" ")] + ([info["eot"]] if 0 <= info["eot"] < n_limit else [])
    return sorted({i for i in out if i >= 0}), sorted({i for i in first if i >= 0})
