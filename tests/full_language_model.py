"""Fixtures of the full-length automatic-language tests (option full_language), and the CPU-oracle
helpers both test files share; nothing here touches the GPU.
Fixture A: lang_model.write_lang_model, then full_model.extend_text_ctx (160 positions), over the clips of
lang_model.lang_mels().  Its text does not depend on the language token (clip 26 under translate aside), but the first
generated token's log-probability does.  Fixture B: A with every decoder.blocks.*.attn.out.weight x 4 — there the text
itself depends on the language token.  tests/test_full_language_reference.py pins what the oracle gives on both."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import full_model as fm  # noqa: E402
import lang_model as lm  # noqa: E402

TRANSLATE = lm.LANG_LO + lm.N_LANG  # 50358 in this vocabulary; lm.TRANSCRIBE = 50359
CLIPS = (0, 22, 26, 31)             # the GPU tests' clips: languages 87, 94, 94, 87
CLIPS8 = (0, 1, 2, 3, 22, 24, 26, 31)
B_LANG = 50                         # what every clip of fixture B detects
B_GAIN = 4.0


def write_a(src_wtw, dst_wtw):
    tmp = dst_wtw + ".lang.tmp"
    lm.write_lang_model(src_wtw, tmp)
    fm.extend_text_ctx(tmp, dst_wtw)
    os.remove(tmp)


def write_b(src_wtw, dst_wtw):
    from wtw import read_wtw, write_wtw
    write_a(src_wtw, dst_wtw)
    dims, t = read_wtw(dst_wtw)
    t = {k: np.array(v) for k, v in t.items()}
    for l in range(dims["n_text_layer"]):
        t[f"decoder.blocks.{l}.attn.out.weight"] *= B_GAIN
    write_wtw(dst_wtw, dict(dims), t)


def prompt_for(lang, task=lm.TRANSCRIBE, timestamps=False):
    p = [lm.SOT, lm.LANG_LO + int(lang), task]
    return p if timestamps else p + [lm.NOTIMESTAMPS]


def decode(model, enc, prompt, positions):
    """Greedy ids behind `prompt`, the smallest top-two margin over the steps, and the log-probability of the first
    generated token under the whole vocabulary."""
    ids, logits = model.decode_greedy(enc, prompt, positions, lm.EOT, True, True, 8, True)
    margin = min(lm.top_two_gap(logits[s]) for s in range(logits.shape[0]))
    z = logits[0].astype(np.float64)
    lp0 = float(z[int(ids[len(prompt)])] - (z.max() + np.log(np.exp(z - z.max()).sum())))
    return [int(i) for i in ids], float(margin), lp0


# The 64 active ids of the fixtures as word pieces without a leading space and without punctuation: whichever of them a
# clip's text holds (the synthetic decoder repeats few ids), Whisper's space rule joins them into one word and the
# unicode_only rule (one word per complete UTF-8 sequence) makes one word of each.
WORD_PIECES = [b"he", b"llo", b"ing", b"s", "語".encode(), b"x", b"wor", b"ld"]


def write_word_vocab(src_vocab, dst_vocab, n_tokens=50257):
    """A vocabulary file with the filters of src_vocab and WORD_PIECES, repeated, at ids 0 .. 63 (every other id "x"):
    [u64 payload bytes][u32 magic][i32 n_mel][i32 n_fft][filters][i32 n_vocab]{u32 length, bytes}."""
    import struct
    raw = open(src_vocab, "rb").read()
    _, n_mel, n_fft = struct.unpack_from("<Iii", raw, 8)
    head = raw[8: 8 + 12 + 4 * n_mel * n_fft]
    payload = head + struct.pack("<i", n_tokens)
    for i in range(n_tokens):
        t = WORD_PIECES[i % len(WORD_PIECES)] if i < 64 else b"x"
        payload += struct.pack("<I", len(t)) + t
    with open(dst_vocab, "wb") as f:
        f.write(struct.pack("<Q", len(payload)) + payload)
