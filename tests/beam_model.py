"""The EOT-rich micro model of the beam-search parity tests: micro dims with the multilingual vocabulary size, so that
the synthetic vocabulary's EOT (50257) and the default prompt exist.  The logits of a random-init model are a dense
cloud over 51865 ids whose top ranks sit ~1e-4 apart, closer than any two implementations agree; here `n_active` ids
get embedding rows `gain` times the original scale and every other row a small one, so the top ranks are whole units apart; the EOT row
is `eot_gain` times as long again, so that EOT competes with them."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VOCAB, EOT = 51865, 50257
PROMPT = [50258, 50261, 50359, 50363]  # the engine's default EncDec prompt (language de)


def write_eot_rich(src_wtw, dst_wtw, eot_gain, gain, n_active, seed=7):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from wtw import read_wtw, write_wtw
    dims, t = read_wtw(src_wtw)
    t = {k: np.asarray(v) for k, v in t.items()}
    d = dict(dims)
    d["n_vocab"] = N_VOCAB
    E = t["decoder.token_embedding.weight"]
    rng = np.random.default_rng(seed)
    E2 = (rng.standard_normal((N_VOCAB, E.shape[1])) * E.std() * 0.05).astype(np.float32)
    E2[:n_active] *= gain / 0.05
    E2[EOT] *= eot_gain * gain / 0.05
    t["decoder.token_embedding.weight"] = E2
    write_wtw(dst_wtw, d, t)
