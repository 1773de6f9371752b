"""Reference for several samples per clip, in float64 numpy.

Sample j of a clip is tests/sample_ref.py's decode (or step) under the attempt word attempt + (j << 16): sample 0 is the
decode that draws one sample.  The kept sample is the FIRST with the largest sum_logprob / n_generated in float64, every
generated id counted, EOT included (section 15's avg_logprob; a sample that reached the cap without EOT counts what it
generated).  A NaN average, or a sample that counted nothing, never wins; where none is left, sample 0 is kept.

Rows of a chain over `clips` clips are laid out r = j * clips + c: sample j of clip c."""
from __future__ import annotations

import math

import numpy as np

N_MAX = 8


def attempt_word(attempt, j):
    """The fourth word of the Philox counter for sample j of an attempt."""
    assert 0 <= j < N_MAX and 0 <= attempt < (1 << 16)
    return int(attempt) + (int(j) << 16)


def average(s, n):
    """sum / count in float64; NaN where nothing was counted."""
    if n < 1:
        return math.nan
    with np.errstate(all="ignore"):
        return float(np.float64(s) / np.float64(n))


def rank(sums, counts):
    """Index of the kept sample among a clip's (sum, count) pairs."""
    best, best_avg = -1, 0.0
    for j, (s, n) in enumerate(zip(sums, counts)):
        a = average(s, int(n))
        if not math.isnan(a) and (best < 0 or a > best_avg):
            best, best_avg = j, a
    return max(best, 0)


def row_of(c, j, clips):
    return j * clips + c


def pick(ids, lp, n_ids, sums, counts, N, c0, out):
    """best_of_pick on numpy arrays: inputs over N * clips rows, `out` a dict of the output arrays (ids, lp, n, count,
    picked, sum, all_sum, all_count) over at least c0 + clips rows.  Returns the changed copy."""
    R, stride = ids.shape
    clips = R // N
    assert clips * N == R
    o = {k: np.array(v, copy=True) for k, v in out.items()}
    for c in range(clips):
        rows = [row_of(c, j, clips) for j in range(N)]
        j = rank(sums[rows], counts[rows])
        r, k = rows[j], c0 + c
        n = min(max(int(n_ids[r]), 0), stride)
        o["ids"][k], o["lp"][k] = 0, 0.0
        o["ids"][k, :n], o["lp"][k, :n] = ids[r, :n], lp[r, :n]
        o["n"][k], o["count"][k], o["picked"][k], o["sum"][k] = n, counts[r], j, sums[r]
        o["all_sum"][k], o["all_count"][k] = 0.0, 0
        o["all_sum"][k, :N], o["all_count"][k, :N] = sums[rows], counts[rows]
    return o


def begin(prompts, n_prompt, N, cap, frozen=None):
    """best_of_begin: prompts int64 [clips][stride] -> (ids [N * clips][stride] with the prompt's first n_prompt ids and
    zeros behind them on the rows j >= 1, rows j = 0 as given; n_ids, finished, sum, count; anc uint8 [N * clips][cap])."""
    clips, stride = prompts.shape
    R = N * clips
    ids = np.zeros((R, stride), np.int64)
    ids[:clips] = prompts
    for r in range(clips, R):
        ids[r, :n_prompt] = prompts[r % clips, :n_prompt]
    fin = np.array([0 if frozen is None else int(bool(frozen[r % clips])) for r in range(R)], np.int32)
    anc = np.zeros((R, cap), np.uint8)
    for r in range(R):
        anc[r, :] = r
        anc[r, : max(n_prompt - 1, 0)] = r % clips
    return ids, np.full(R, n_prompt, np.int32), fin, np.zeros(R, np.float64), np.zeros(R, np.int32), anc


def decode_samples(decode_at, N, attempt=0):
    """decode_at(attempt_word) -> sample_ref.decode's dict.  Returns (picked, rows): the N samples of one attempt and the
    index of the kept one."""
    rows = [decode_at(attempt_word(attempt, j)) for j in range(N)]
    return rank([r["sum"] for r in rows], [r["n"] for r in rows]), rows
