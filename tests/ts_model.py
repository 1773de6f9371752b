"""Model of the timestamp decoding tests (option timestamps): the EOT-rich micro model of
tests/full_model.py (multilingual vocabulary size, n_text_ctx raised, loud text rows and a louder EOT row) whose 1501
timestamp rows [beg, n_vocab) are scaled by TS_GAIN, so that the summed probability of the timestamps competes with the
text ids: on some steps one timestamp logit beats every text logit, on others only their sum does (rule 5), and mostly
text wins.  The gains, seed and clip count were chosen on the CPU; tests/test_ts_reference.py pins what they give."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import beam_model  # noqa: E402
import full_model  # noqa: E402
import ts_ref  # noqa: E402

N_VOCAB, EOT = beam_model.N_VOCAB, beam_model.EOT
BEG = 50364                       # <|0.00|> of the multilingual vocabulary; n_vocab - BEG = 1501 ticks
PROMPT = beam_model.PROMPT[:3]    # the engine's default prompt with timestamps: [sot, <|de|>, transcribe]
N_TEXT_CTX = 128
P_LONG, P_SHORT = 96, 40          # positions fed; 40 ends inside the second 32-position segment
RICH = (6.0, 40.0, 64)            # write_eot_rich's eot_gain, gain, n_active (as tests/full_model.py)
TS_GAIN = 1300.0                  # the timestamp rows' scale, in units of the quiet rows' (1.6 x the loud text rows')
SEED, CLIPS = 21, 10
LOOKAHEAD = 12
MARGIN = 2e-4                     # the decisive-margin rule: twice the logits bar


def write_model(src_wtw, dst_wtw, ts_gain=TS_GAIN, rich=RICH):
    from wtw import read_wtw, write_wtw
    full_model.write_eot_rich(src_wtw, dst_wtw, rich[0], rich[1], rich[2], n_text_ctx=N_TEXT_CTX)
    dims, t = read_wtw(dst_wtw)
    t = {k: np.array(v) for k, v in t.items()}
    t["decoder.token_embedding.weight"][BEG:] *= np.float32(ts_gain)
    write_wtw(dst_wtw, dims, t)


def mels(n=CLIPS, shape=(80, 200), seed=SEED):
    return full_model.mels(n, shape, seed)


def logits_fn(model, enc_out, max_pos):
    """Next-token logits of a prefix from the CPU oracle.  The oracle evaluates one prefix per call; a call therefore
    decodes on greedily (unfiltered) for up to LOOKAHEAD positions and keeps those steps' logits under the prefixes they
    belong to: as long as the filtered choice equals the plain argmax the next prefix is already there.  Prefixes only
    grow, so shorter ones are dropped."""
    memo = {}

    def fn(prefix):
        key = tuple(int(i) for i in prefix)
        if key not in memo:
            for old in [k for k in memo if len(k) < len(key)]:
                del memo[old]
            ids, lg = model.decode_greedy(enc_out, list(key), max_positions=max(min(max_pos, len(key) + LOOKAHEAD), len(key)),
                                          eot=EOT, stop_at_eot=False, want_logits=True)
            ids = [int(i) for i in ids]
            for k in range(lg.shape[0]):
                memo.setdefault(tuple(ids[: len(key) + k]), np.asarray(lg[k], np.float32).copy())
        return memo[key]

    return fn


def reference_rows(model, mel, max_pos, prompt=PROMPT, max_initial=50):
    """Per clip: ts_ref.decode over the oracle -> (ids, infos)."""
    rows = []
    for b in range(mel.shape[0]):
        fn = logits_fn(model, model.encode(mel[b]), max_pos)
        rows.append(ts_ref.decode(fn, prompt, max_pos, EOT, BEG, max_initial))
    return rows


def cut_rows(rows, max_pos, n_prompt=len(PROMPT)):
    """The rows of a decode over max_pos positions from those of a longer one: every step depends on its prefix alone,
    so the shorter decode is the longer one cut after max_pos + 1 ids."""
    return [(ids[: max_pos + 1], infos[: max_pos + 1 - n_prompt]) for ids, infos in rows]
