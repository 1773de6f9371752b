"""The input resampler's specification (include/wt_capi.h) restated in float64 numpy: the
Hann-windowed sinc polyphase filter, any rate -> 16 kHz."""
import math

import numpy as np

LPW, ROLLOFF, OUT_RATE = 6, 0.99, 16000


def plan(rate):
    """(orig, new, w, K)"""
    g = math.gcd(rate, OUT_RATE)
    orig, new = rate // g, OUT_RATE // g
    w = int(math.ceil(LPW * orig / (min(orig, new) * ROLLOFF)))
    return orig, new, w, 2 * w + orig


def filt(rate):
    """h [new][K]"""
    orig, new, w, K = plan(rate)
    base = min(orig, new) * ROLLOFF
    k = np.arange(K, dtype=np.float64)[None, :]
    p = np.arange(new, dtype=np.float64)[:, None]
    a = np.pi * np.clip(((k - w) / orig - p / new) * base, -LPW, LPW)
    sinc = np.where(a == 0, 1.0, np.sin(a) / np.where(a == 0, 1.0, a))
    c = np.cos(a / (2.0 * LPW))
    return sinc * (c * c) * (base / orig)


def out_len(rate, n):
    orig, new, _, _ = plan(rate)
    return -(-new * n // orig)


def _apply(h, x, rate):
    orig, new, w, K = plan(rate)
    n_out = out_len(rate, len(x))
    blocks = -(-n_out // new)
    xp = np.zeros(w + blocks * orig + K, np.float64)
    xp[w:w + len(x)] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, K)[::orig][:blocks]  # [i][k] = x[i orig + k - w]
    return (win @ h.T).reshape(-1)[:n_out]


def resample(x, rate):
    return _apply(filt(rate), np.asarray(x, np.float64), rate)


def abs_sum(x, rate):
    """S[j] = sum_k |h| |x| of output j: what a rounding-error bound is relative to"""
    return _apply(np.abs(filt(rate)), np.abs(np.asarray(x, np.float64)), rate)
