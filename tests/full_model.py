"""Models of the full-length decoding tests (option max_positions): the micro weights with
n_text_ctx raised from 64 to 160 — extra positional rows drawn with the std of the existing ones.  160 positions cross
the 31-position limit of the max_tokens path and two 64-key tiles of self_attention_long, and the micro-dims oracle
still decodes them on the CPU in seconds.  Two flavours: the dense random-init model (micro vocabulary, 1024 ids, never
an EOT) and an EOT-rich one (beam_model.write_eot_rich: multilingual vocabulary size, `n_active` loud ids and a louder
EOT row).  In a random-init decoder the position, not the clip, decides where EOT first wins — every clip of a batch then
finishes within a few positions of the others — so the EOT-rich flavour also sharpens the decoder's cross-attention
(query weights x CROSS_Q_GAIN) and doubles its share of the residual stream (out weights x CROSS_OUT_GAIN): what a clip
sounds like then moves its finishing position from 17 to never."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import beam_model  # noqa: E402

N_TEXT_CTX = 160
DENSE_PROMPT = [3, 5, 7, 11]  # the micro vocabulary has no multilingual special ids
RICH_PROMPT = beam_model.PROMPT
EOT = beam_model.EOT
# write_eot_rich (eot_gain, gain, n_active) and the mel seed / clip count of the EOT-rich tests, chosen on the CPU
# (tests/test_full_reference.py pins what they give): clips that finish before position 32, between 33 and 159, and never
RICH = (6.0, 40.0, 64)
CROSS_Q_GAIN, CROSS_OUT_GAIN = 4.0, 2.0
RICH_SEED, RICH_CLIPS = 21, 12
# the dense flavour's six clips: those of a pool of 30 whose smallest top-two margin over 157 steps on the oracle is
# above 3e-4 (the pool's margins run from 5e-6 to 1e-3: a 1024-id random-init vocabulary is a dense cloud)
DENSE_SEED, DENSE_POOL, DENSE_PICK = 1234, 30, (2, 5, 8, 9, 18, 19)
MARGIN = 2e-4  # the decisive-margin rule: twice the logits bar, as tests/test_gpu_beam.py


def extend_text_ctx(src_wtw, dst_wtw, n_text_ctx=N_TEXT_CTX, seed=11):
    from wtw import read_wtw, write_wtw
    dims, t = read_wtw(src_wtw)
    t = {k: np.array(v) for k, v in t.items()}
    d = dict(dims)
    pos = t["decoder.positional_embedding"]
    assert pos.shape[0] == d["n_text_ctx"] <= n_text_ctx
    rng = np.random.default_rng(seed)
    extra = (rng.standard_normal((n_text_ctx - pos.shape[0], pos.shape[1])) * pos.std()).astype(np.float32)
    t["decoder.positional_embedding"] = np.concatenate([pos, extra], axis=0)
    d["n_text_ctx"] = n_text_ctx
    write_wtw(dst_wtw, d, t)


def write_dense(src_wtw, dst_wtw, n_text_ctx=N_TEXT_CTX):
    extend_text_ctx(src_wtw, dst_wtw, n_text_ctx)


def write_eot_rich(src_wtw, dst_wtw, eot_gain=RICH[0], gain=RICH[1], n_active=RICH[2], n_text_ctx=N_TEXT_CTX):
    from wtw import read_wtw, write_wtw
    tmp = dst_wtw + ".tmp"
    beam_model.write_eot_rich(src_wtw, tmp, eot_gain, gain, n_active)
    extend_text_ctx(tmp, dst_wtw, n_text_ctx)
    os.remove(tmp)
    dims, t = read_wtw(dst_wtw)
    t = {k: np.array(v) for k, v in t.items()}
    for l in range(dims["n_text_layer"]):
        t[f"decoder.blocks.{l}.cross_attn.query.weight"] *= CROSS_Q_GAIN
        t[f"decoder.blocks.{l}.cross_attn.out.weight"] *= CROSS_OUT_GAIN
    write_wtw(dst_wtw, dims, t)


def mels(n, shape, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.5, size=(n,) + tuple(shape)).astype(np.float32)


def dense_mels(shape):
    return np.ascontiguousarray(mels(DENSE_POOL, shape, DENSE_SEED)[list(DENSE_PICK)])


def oracle_rows(model, mel, prompt, max_positions, eot, stop_at_eot=True):
    """Per clip: the oracle's greedy ids and the top-two logit margin of every step (its logits, last-maximum rule)."""
    rows = []
    for b in range(mel.shape[0]):
        ids, logits = model.decode_greedy(model.encode(mel[b]), prompt, max_positions, eot, stop_at_eot, True, 8, True)
        top2 = np.partition(logits, -2, axis=1)[:, -2:]
        rows.append(([int(i) for i in ids], (top2[:, 1] - top2[:, 0]).astype(np.float64)))
    return rows


def finish_index(ids, eot=EOT):
    """Index of the EOT that ended the row, or None when the clip ran to the cap."""
    return len(ids) - 1 if ids[-1] == eot else None


def first_indecisive(margins, bar=MARGIN):
    """Index into the id row of the first token chosen with a top-two margin below `bar` (None: every step decisive);
    step s chooses ids[n_prompt + s]."""
    low = np.nonzero(np.asarray(margins) < bar)[0]
    return int(low[0]) if low.size else None
