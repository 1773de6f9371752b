"""Models of the decode-confidence tests (option scores): the timestamp model of tests/ts_model.py
and the EOT-rich model of tests/full_model.py, each with the <|nospeech|> embedding row (50362 in the multilingual
vocabulary) scaled by a gain.

In these random-init models that row is one of the quiet ones.  Its position-0 logit is about -0.012 for every clip,
against a log-sum-exp over the rest of the vocabulary of 46 .. 51 in the timestamp model and 16 .. 18 in the EOT-rich
one.  The gains are negative, so that the logit turns positive.  NOSP_GAIN puts the no-speech probabilities of the ten
timestamp clips on both sides of NO_SPEECH_THRESHOLD; NOSP_GAIN_PLAIN puts those of the EOT-rich clips between 0.002
and 0.06.

The id lies between EOT and <|0.00|>, which the timestamp rules always mask, so the timestamp model's ids stay those of
tests/ts_model.py.  Gains and thresholds were chosen on the CPU; tests/test_scores_reference.py pins what they give."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import full_model  # noqa: E402
import scores_ref  # noqa: E402
import ts_model  # noqa: E402

NOSP = 50362                      # <|nospeech|>: the vocabulary's token_solm, multilingual
NOSP_GAIN = -4000.0               # the timestamp model: position-0 logit about +48, no_speech_prob from 0.007 to 0.9998
NOSP_GAIN_PLAIN = -1000.0         # the EOT-rich model (log-sum-exp about 17 there): no_speech_prob from 0.002 to 0.06
NO_SPEECH_THRESHOLD = 600         # thousandths: the option's default
LOGPROB_THRESHOLD = -250          # thousandths: between the avg_logprob of the clips above the no-speech threshold
EOT, BEG = ts_model.EOT, ts_model.BEG
TS_PROMPT, PLAIN_PROMPT = ts_model.PROMPT, full_model.RICH_PROMPT
P_LONG, P_SHORT = ts_model.P_LONG, ts_model.P_SHORT
P_PLAIN = 96                      # three 32-position segments; clips end before 32, later, and at the cap
MARGIN = ts_model.MARGIN


def _scale_nosp(wtw_path, gain):
    from wtw import read_wtw, write_wtw
    dims, t = read_wtw(wtw_path)
    t = {k: np.array(v) for k, v in t.items()}
    t["decoder.token_embedding.weight"][NOSP] *= np.float32(gain)
    write_wtw(wtw_path, dims, t)


def write_ts_model(src_wtw, dst_wtw, gain=NOSP_GAIN):
    ts_model.write_model(src_wtw, dst_wtw)
    _scale_nosp(dst_wtw, gain)


def write_plain_model(src_wtw, dst_wtw, gain=NOSP_GAIN_PLAIN):
    full_model.write_eot_rich(src_wtw, dst_wtw)
    _scale_nosp(dst_wtw, gain)


def ts_mels():
    return ts_model.mels()


def plain_mels():
    return full_model.mels(full_model.RICH_CLIPS, (80, 200), full_model.RICH_SEED)


def reference(model, mel, max_pos, timestamps):
    """Per clip: scores_ref.decode over the CPU oracle."""
    out = []
    for b in range(mel.shape[0]):
        fn = ts_model.logits_fn(model, model.encode(mel[b]), max_pos)
        out.append(scores_ref.decode(fn, TS_PROMPT if timestamps else PLAIN_PROMPT, max_pos, EOT, NOSP, BEG, timestamps))
    return out


def cut(ref, max_pos, n_prompt):
    """The reference of a decode over max_pos positions from that of a longer one (every step depends on its prefix)."""
    out = []
    for r in ref:
        ids, lps = r["ids"][: max_pos + 1], r["lps"][: max_pos + 1 - n_prompt]
        s = float(np.sum(np.asarray(lps, np.float64)))
        out.append(dict(r, ids=ids, lps=lps, sum=s, n=len(lps), avg=s / len(lps)))
    return out
