"""The language model of the spoken-language tests: beam_model.write_eot_rich on the micro weights
(seed 7, vocabulary 51865, background rows x 0.05, rows 0..63 x 40, EOT row x 3.3 * 40) with the 99 language rows
50259..50357 scaled like the active rows, so that the language logits sit whole units apart, and a mel generator whose
clips differ in level and spread, so that one batch holds more than one language.  CPU-oracle helpers for both test
files live here too; nothing in this module touches the GPU."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_model  # noqa: E402

N_VOCAB, EOT, SOT = beam_model.N_VOCAB, beam_model.EOT, 50258
LANG_LO, N_LANG = 50259, 99
TRANSCRIBE, NOTIMESTAMPS = 50359, 50363
EOT_GAIN, GAIN, N_ACTIVE = 3.3, 40.0, 64
MEL_SEED, N_CLIPS = 4321, 32
# what the CPU oracle gives for the 32 clips (tests/test_lang_reference.py asserts it, so the fixture cannot drift)
EXPECT_LANGS = [94 if b in (22, 24, 26) else 87 for b in range(N_CLIPS)]


def write_lang_model(src_wtw, dst_wtw):
    beam_model.write_eot_rich(src_wtw, dst_wtw, EOT_GAIN, GAIN, N_ACTIVE)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from wtw import read_wtw, write_wtw
    dims, t = read_wtw(dst_wtw)
    t = {k: np.asarray(v) for k, v in t.items()}
    E = t["decoder.token_embedding.weight"].copy()
    E[LANG_LO:LANG_LO + N_LANG] *= GAIN / 0.05
    t["decoder.token_embedding.weight"] = E
    write_wtw(dst_wtw, dict(dims), t)


def lang_mels(n=N_CLIPS, shape=(80, 200), seed=MEL_SEED):
    rng = np.random.default_rng(seed)
    out = np.zeros((n,) + tuple(shape), np.float32)
    for b in range(n):
        a = rng.uniform(-1.0, 1.0)
        s = rng.uniform(0.1, 1.5)
        out[b] = np.clip(a + s * rng.standard_normal(shape), -1.0, 1.5).astype(np.float32)
    return out


def prompt_for(lang):
    return [SOT, LANG_LO + int(lang), TRANSCRIBE, NOTIMESTAMPS]


def argmax_last(x):
    x = np.asarray(x)
    return int(len(x) - 1 - np.argmax(x[::-1]))


def top_two_gap(z):
    s = np.partition(np.asarray(z, np.float64), -2)
    return float(s[-1] - s[-2])


def softmax64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max())
    return e / e.sum()


def oracle_language(model, enc):
    """The oracle's language logits of one clip: the first step of a greedy decode of [sot], columns of the language
    tokens.  Returns (logits float32 [99], lang by argmax_last, top-two gap)."""
    _, logits = model.decode_greedy(enc, [SOT], max_positions=2, eot=EOT, want_logits=True)
    z = logits[0, LANG_LO:LANG_LO + N_LANG].copy()
    return z, argmax_last(z), top_two_gap(z)


def oracle_decode(model, enc, lang, max_positions=30):
    """Greedy decode behind the clip's own prompt: (ids, smallest top-two logit margin over the steps)."""
    ids, logits = model.decode_greedy(enc, prompt_for(lang), max_positions, EOT, True, True, 8, True)
    margin = min(top_two_gap(logits[s]) for s in range(logits.shape[0]))
    return [int(i) for i in ids], margin
