"""CPU: the host fold of the absorbed cross-attention's query side (absorbed_query_matrix, engine.cpp) through its
tap wt_dbg_absorbed_query_matrix: A_h = c0 Wk_h^T Wq_h and a_h = c0 Wk_h^T bq_h with c0 = d_head^-1/2 log2 e, against
a float64 numpy fold, and the identity the absorbed decoder chain rests on ("What the absorbed
chain's tests pin")."""
import numpy as np
import pytest

C0 = 0.125 * np.log2(np.e)


def fold64(wq, bq, wk, heads):
    d = wq.shape[0]
    wq, bq, wk = (np.asarray(a, np.float64) for a in (wq, bq, wk))
    A = np.zeros((heads * d, d))
    a = np.zeros(heads * d)
    for h in range(heads):
        sl = slice(64 * h, 64 * h + 64)
        A[h * d:(h + 1) * d] = C0 * (wk[sl].T @ wq[sl])
        a[h * d:(h + 1) * d] = C0 * (wk[sl].T @ bq[sl])
    return A, a


def draw(heads, seed):
    rng = np.random.default_rng(seed)
    d = 64 * heads
    wq = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    wk = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    bq = rng.standard_normal(d).astype(np.float32)
    return wq, bq, wk


@pytest.mark.parametrize("heads", [2, 6, 8])
def test_fold_is_the_float64_fold_rounded_once(pkg, heads):
    """The fold accumulates in double and rounds each entry to fp32 once, so it may differ from the float64 value by the
    rounding itself (half an ulp) plus the last bits of a differently ordered double sum: at most 1 ulp of the entry.
    A fold without c0 is off by a factor 5.5, one without a_h returns zeros for it."""
    wq, bq, wk = draw(heads, 11 + heads)
    A, a = pkg.absorbed_query_matrix(wq, bq, wk)
    A64, a64 = fold64(wq, bq, wk, heads)
    d = 64 * heads
    assert A.shape == (heads * d, d) and a.shape == (heads * d,)
    assert A.dtype == np.float32 and a.dtype == np.float32
    assert (np.abs(A - A64) <= np.spacing(np.abs(A64).astype(np.float32))).all()
    assert (np.abs(a - a64) <= np.spacing(np.abs(a64).astype(np.float32))).all()
    assert np.abs(a64).min() > 0 and np.abs(a).min() > 0


@pytest.mark.parametrize("heads", [2, 6, 8])
def test_absorbed_scores_are_the_scaled_textbook_scores(pkg, heads):
    """(A_h y + a_h) . e = c0 (Wq_h y + bq_h) . (Wk_h e) for any y, e (the key projection has no bias).  The right side
    is float64 on the fp32 weights; the left uses the tap's fp32 A, a in float64 arithmetic, so the only difference is
    the one rounding of every entry of A and a: |diff| <= 2^-24 (|A_h| |y| + |a_h|) . |e|, asserted with a margin of 2."""
    wq, bq, wk = draw(heads, 23 + heads)
    A, a = pkg.absorbed_query_matrix(wq, bq, wk)
    d = 64 * heads
    rng = np.random.default_rng(heads)
    for _ in range(8):
        y, e = rng.standard_normal(d), rng.standard_normal(d)
        for h in range(heads):
            sl = slice(64 * h, 64 * h + 64)
            Ah, ah = A[h * d:(h + 1) * d].astype(np.float64), a[h * d:(h + 1) * d].astype(np.float64)
            lhs = (Ah @ y + ah) @ e
            rhs = C0 * ((wq[sl].astype(np.float64) @ y + bq[sl]) @ (wk[sl].astype(np.float64) @ e))
            bound = 2.0 * 2.0 ** -24 * ((np.abs(Ah) @ np.abs(y) + np.abs(ah)) @ np.abs(e))
            assert abs(lhs - rhs) <= bound, (h, lhs, rhs, bound)
            assert abs(rhs) > 0


def test_fold_refuses_a_width_that_is_not_64_per_head(pkg):
    import ctypes
    z = np.zeros(4, np.float32)
    fp = z.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert pkg.lib().wt_dbg_absorbed_query_matrix(2, 100, fp, fp, fp, fp, fp) == 1  # WT_ERR_INVALID_ARG
    assert pkg.lib().wt_dbg_absorbed_query_matrix(0, 0, fp, fp, fp, fp, fp) == 1
