"""Reference truncated sampling (options top_k / top_p) in float64, ties by exact integer keys:
A ordered by key = ord(z_i) << 32 | i descending, K its first min(top_k, |A|) ids, N the shortest prefix of K with
sum p >= top_p * sum over K, p_i = exp((z_i - m) * inv_t); cut = the key of N's last id.  step: sample_ref's Gumbel
maximum over N; rule 5 on all allowed ids; a class it leaves with no id in N yields its largest unperturbed key."""
import math

import numpy as np

import sample_ref as sr
import scores_ref


def keys_of(z):
    u = np.asarray(z, np.float32).view(np.uint32).astype(np.uint64)
    o = np.where(u & 0x80000000 != 0, np.where(u == 0x80000000, 0x80000000, ~u & 0xFFFFFFFF), u | 0x80000000).astype(np.uint64)
    return (o << np.uint64(32)) | np.arange(u.size, dtype=np.uint64)


def cut(z, allowed, T, top_k=0, top_p=1.0):
    """-> cut, kept, N, K (ids in key order), ratio (mass of N / mass of A), margin (distance of the mass of N, and of
    N without its last id, from the target, over the mass of K; inf with top_p off)."""
    z, keys = np.asarray(z, np.float32), keys_of(z)
    A = np.flatnonzero(allowed)
    A = A[np.argsort(keys[A])[::-1]]
    K = A[:min(int(top_k), A.size)] if top_k > 0 else A
    with np.errstate(invalid="ignore"):
        pa = np.exp((z[A].astype(np.float64) - np.float64(z[A].max())) * np.float64(sr.inv_t_of(T)))
    c, top_p = np.cumsum(pa[:K.size]), float(np.float32(top_p))
    n, margin = K.size, math.inf
    if 0.0 < top_p < 1.0:
        target = top_p * c[-1]
        n = int(np.searchsorted(c, target, side="left")) + 1  # the first prefix whose mass is >= the target
        margin = min(c[n - 1] - target, target - (c[n - 2] if n > 1 else 0.0)) / c[-1]
    return {"cut": int(keys[K[n - 1]]), "kept": n, "N": K[:n], "K": K, "ratio": float(c[n - 1] / pa.sum()), "margin": float(margin)}


def rule_mask(z, g, eot, beg, max_initial, timestamps):
    """The ids rules 1 .. 4 allow: the set the cut is taken over."""
    mask = np.ones(np.asarray(z).size, bool)
    if timestamps:
        t_lo, t_hi, s_lo, s_hi = scores_ref.intervals(list(g), mask.size, eot, beg, max_initial)
        mask[:] = False
        mask[t_lo:t_hi + 1] = mask[s_lo:s_hi + 1] = True
    return mask


def step(z, g, T, top_k, top_p, seed=0, pos=0, clip=0, attempt=0, eot=0, beg=0, max_initial=50, timestamps=False):
    """One truncated sampling step -> (token, info): N, gap and bar as sample_ref.step's, fallback (item 4), mass."""
    z = np.asarray(z, np.float32)
    ref = cut(z, rule_mask(z, g, eot, beg, max_initial, timestamps), T, top_k, top_p)
    chosen, tsi = sr.allowed_mask(z, g, eot, beg, max_initial, timestamps)
    idx = np.intersect1d(np.flatnonzero(chosen), ref["N"])
    info = {"N": ref["N"], "gap": math.inf, "bar": 0.0, "fallback": idx.size == 0, "mass": bool(tsi and tsi["mass"])}
    if idx.size == 0:
        cls = np.flatnonzero(chosen)
        return int(cls[np.argmax(keys_of(z)[cls])]), info
    gum = sr.gumbel_of(sr.uniform_of(sr.words(z.size, pos, clip, attempt, seed)[idx]))
    k = z[idx].astype(np.float64) * np.float64(sr.inv_t_of(T)) + gum
    best = int(np.flatnonzero(k == k.max())[-1])
    if idx.size > 1:
        second = int(np.argmax(np.where(np.arange(idx.size) == best, -np.inf, k)))
        info["gap"] = float(k[best] - k[second])
        info["bar"] = sr.key_bar(k[best], gum[best]) + (sr.key_bar(k[second], gum[second]) if np.isfinite(k[second]) else 0.0)
    return int(idx[best]), info
