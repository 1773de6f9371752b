"""Host only: the truncated-sampling entry points are exported and declared, and tests/nucleus_ref.py keeps its own
invariants: N is never empty, N is a prefix of K and K of A in key order, and N grows with top_p."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nucleus_ref as nr  # noqa: E402


def test_symbols_are_exported_and_declared(pkg):
    header = open(os.path.join(ROOT, "include", "wt_debug.h")).read()
    for sym in ("wt_dbg_nucleus_cut", "wt_dbg_sample_select_cut"):
        assert sym in pkg.DEBUG_SYMBOLS and f"int {sym}(" in header and getattr(pkg.lib(), sym)
    capi = open(os.path.join(ROOT, "include", "wt_capi.h")).read()
    assert '"top_k"' in capi and '"top_p"' in capi


def test_reference_invariants():
    rng = np.random.default_rng(1)
    for V in [5] * 10 + [300] * 10:
        z = (rng.standard_normal(V) * 3).astype(np.float32)
        z[rng.integers(0, V, V // 5)] = -np.inf
        z[rng.integers(0, V, 3)] = z[0]  # ties
        allowed = rng.random(V) < 0.7
        allowed[int(np.argmax(np.where(np.isfinite(z), z, -1e9)))] = True  # a finite maximum inside A
        T, top_k, keys, last = float(rng.choice([0.3, 1.0])), int(rng.choice([0, 1, 3, V + 2])), nr.keys_of(z), 0
        for top_p in (0.001, 0.3, 0.6, 0.9, 0.999, 1.0):
            ref = nr.cut(z, allowed, T, top_k, top_p)
            N, K = list(ref["N"]), list(ref["K"])
            assert 1 <= len(N) and N == K[:len(N)] and len(K) == (min(top_k, allowed.sum()) if top_k else allowed.sum())
            assert allowed[K].all() and all(keys[K[i]] > keys[K[i + 1]] for i in range(len(K) - 1))
            assert set(N) == {i for i in np.flatnonzero(allowed) if keys[i] >= ref["cut"]} and ref["kept"] == len(N) >= last
            last = len(N)
        assert last == len(K)  # top_p = 1: off
