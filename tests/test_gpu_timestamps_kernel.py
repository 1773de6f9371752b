"""GPU (-m gpu): ts_partial + ts_select of csrc/k_timestamps.hip (option timestamps) through the
debug tap wt_dbg_timestamp_select, one step per row, against tests/ts_ref.py: every rule on hand-set tables, ties and
-inf, ranges of one id, eot / beg at, before and behind a 4096-entry chunk boundary, 0, 1 and 2 generated ids, tick 1500,
row independence, 1, 3 and 64 rows, and the accuracy of rule 5's logsumexp against float64 numpy."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ts_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SB = 2  # sample_begin of every row here: a two-id prompt
# |L - float64 L|, measured: 1.0e-7 over the cases of test_logsumexp_accuracy; the bound is five
# times that.  (The chunk sums are fp32 — expf within 2 ulp, its argument v - m rounded to fp32, at most 24 additions on
# an entry's path: 2.7e-6 relative at the very worst, which is the absolute error of the logarithm — and the merge of the
# chunks is float64.)  Far below 1e-4, half the decisive margin.
L_BOUND = 5e-7


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def run(eng, z, gens, eot, beg, mit=50):
    """One step per row: logits z [B][V], generated ids gens[b] behind the prompt [1, 1]; checks token, L and M of every
    row against ts_ref.step and returns (tokens, L, M)."""
    z = np.ascontiguousarray(z, np.float32)
    B = z.shape[0]
    stride = SB + max(len(g) for g in gens) + 1
    ids = np.zeros((B, stride), np.int64)
    ids[:, :SB] = 1
    n = np.zeros(B, np.int32)
    for b, g in enumerate(gens):
        ids[b, SB:SB + len(g)] = g
        n[b] = SB + len(g)
    tok, L, M = eng.dbg_timestamp_select(z, ids, n, SB, eot, beg, mit)
    for b, g in enumerate(gens):
        want, info = ts_ref.step(z[b], list(g), eot, beg, mit)
        assert int(tok[b]) == want, (b, int(tok[b]), want, info)
        if info["L"] is None:
            assert np.isnan(L[b])
        elif info["L"] == -np.inf:
            assert L[b] == -np.inf
        else:
            assert abs(L[b] - info["L"]) <= L_BOUND, (b, L[b], info["L"])
        if info["M"] is None:
            assert np.isnan(M[b])
        else:
            assert M[b] == np.float32(info["M"])
    return tok, L, M


def rand(rng, B, V, scale=1.0):
    return (rng.standard_normal((B, V)) * scale).astype(np.float32)


def test_each_rule_on_hand_set_tables(eng):
    V, EOT, BEG = 20, 6, 10

    def table(**at):
        z = np.full(V, -5.0, np.float32)
        for k, v in at.items():
            z[int(k[1:])] = v
        return z
    cases = [  # (logits, generated ids, max_initial, expected token)
        (table(i8=9.0, i3=1.0), [BEG + 1, 2], 50, 3),                       # rule 1
        (table(i15=9.0, i2=1.0), [BEG + 1], 50, 2),                         # rule 2: text after the opening timestamp
        (table(i15=9.0, i2=1.0), [BEG + 1, 3, BEG + 4, BEG + 4], 50, 2),    #         ... and after a pair
        (table(i2=9.0, i15=1.0), [BEG + 1, 3, BEG + 4], 50, BEG + 5),       #         text forbidden
        (table(i2=9.0, i6=8.0, i15=1.0), [BEG + 1, 3, BEG + 4], 50, EOT),   #         EOT is not
        (table(i12=9.0, i14=3.0, i15=2.0), [BEG + 1, 3, BEG + 4], 50, BEG + 4),            # rule 3, closing: >= t
        (table(i12=9.0, i14=3.0, i15=2.0), [BEG + 1, 3, BEG + 4, BEG + 4, 2], 50, BEG + 5),  #      after text: > t
        (table(i1=1.0), [BEG + 9, 3], 50, 1),                               # the last tick reached: no timestamp left
        (table(i1=1.0), [BEG + 1, 3, BEG + 9], 50, BEG + 9),                # ... but the pair may close on it
        (table(i2=9.0, i6=8.0, i17=7.0, i12=1.0, i13=1.0), [], 3, BEG + 3),  # rule 4, and a tie: the larger id
        (table(i2=9.0, i6=8.0, i17=7.0), [], -1, BEG + 7),
        (table(i2=9.0, i6=8.0, i17=7.0), [], 0, BEG),
    ]
    for z, g, mit, want in cases:  # (rows of one launch share their step count: one call per case)
        tok, _, _ = run(eng, z[None], [g], EOT, BEG, mit)
        assert int(tok[0]) == want, (g, int(tok[0]), want)
    # rule 5: ten timestamps at 0 against a text logit of 1 (log 9 = 2.20 > 1), then of 2.5
    z = table(i2=1.0)
    z[BEG:] = 0.0
    tok, L, M = run(eng, z[None], [[BEG, 3]], EOT, BEG)
    assert int(tok[0]) == BEG + 9 and abs(L[0] - np.log(9.0)) < 1e-6 and M[0] == 1.0
    z[2] = 2.5
    assert int(run(eng, z[None], [[BEG, 3]], EOT, BEG)[0][0]) == 2
    # L == M exactly: not above, text stays, and the tie goes to the larger id
    z = table(i2=1.0, i12=1.0)
    z[BEG:BEG + 2] = -np.inf
    z[BEG + 3:] = -np.inf
    tok, L, M = run(eng, z[None], [[BEG, 3]], EOT, BEG)
    assert int(tok[0]) == BEG + 2 and L[0] == 1.0 and M[0] == 1.0


def test_ties_signed_zeros_and_minus_infinity(eng):
    V, EOT, BEG = 20, 6, 10
    z = np.full(V, -1.0, np.float32)
    z[1], z[4] = 0.0, -0.0
    assert int(run(eng, z[None], [[BEG + 9, 2]], EOT, BEG)[0][0]) == 4
    z[1], z[4] = -0.0, 0.0
    assert int(run(eng, z[None], [[BEG + 9, 2]], EOT, BEG)[0][0]) == 4
    z = np.full(V, -np.inf, np.float32)  # every logit -inf: the largest allowed id
    assert int(run(eng, z[None], [[BEG + 9, 2]], EOT, BEG)[0][0]) == EOT
    assert int(run(eng, z[None], [[]], EOT, BEG, 4)[0][0]) == BEG + 4
    tok, L, _ = run(eng, z[None], [[BEG + 1, 2]], EOT, BEG)  # timestamps allowed, all -inf: L = -inf, not above M
    assert L[0] == -np.inf and int(tok[0]) == V - 1
    rng = np.random.default_rng(0)
    z = rand(rng, 3, 4101)
    z[:, rng.integers(0, 4101, 2000)] = -np.inf  # -inf scattered over text and timestamps
    z[1] = np.round(z[1])  # many exact ties
    run(eng, z, [[4000, 5]] * 3, 3000, 3990)


def test_ranges_of_one_id(eng):
    rng = np.random.default_rng(1)
    z = rand(rng, 3, 4101)
    for g in ([], [4100], [4100, 4100], [4100, 7], [4100, 7, 4100]):
        run(eng, z, [g] * 3, 4098, 4100)  # one timestamp: beg = V - 1
    for g in ([], [5], [5, 5], [5, 0], [5, 0, 9]):
        run(eng, z, [g] * 3, 0, 1)        # text is EOT alone: eot = 0, beg = 1


@pytest.mark.parametrize("V", [4101, 8192, 51865])
def test_chunk_boundaries_and_generated_lengths(eng, V):
    """eot and beg at, before and behind a chunk boundary; 0, 1 and 2 (and more) generated ids; the timestamp logits
    raised so that rule 5 goes both ways."""
    rng = np.random.default_rng(V)
    edges = [4096] if V == 4101 else ([4096, 8190] if V == 8192 else [4096, 49152, 50364])
    for edge in edges:
        for beg in (edge - 1, edge, edge + 1):
            for eot in (beg - 1, beg - 3, 4095 if beg > 4100 else 1):
                z = rand(rng, 3, V)
                z[:, beg:] += np.float32(rng.choice([-2.0, 2.0, 6.0]))
                t = [min(beg + d, V - 1) for d in (0, 1, 2, 3)]
                for g in ([], [t[0]], [3], [t[1], t[1]], [t[0], 3], [3, t[1]], [t[0], 3, t[2]], [t[0], 3, t[2], t[2], 4]):
                    run(eng, z, [g] * 3, eot, beg, mit=int(rng.choice([-1, 0, 1, 50])))


def test_tick_1500(eng):
    V, EOT, BEG = 51865, 50257, 50364
    rng = np.random.default_rng(2)
    z = rand(rng, 3, V)
    z[:, BEG:] += 8.0
    last = V - 1
    assert last - BEG == 1500
    tok, L, _ = run(eng, z, [[BEG, 5, last]] * 3, EOT, BEG)   # closing: only tick 1500 is left
    assert (tok == last).all() or (tok == EOT).all()
    tok, L, _ = run(eng, z, [[BEG, 5, last, last, 7]] * 3, EOT, BEG)  # behind it: no timestamp is allowed
    assert np.isnan(L).all() and (tok <= EOT).all()
    tok, _, _ = run(eng, z, [[BEG, 5, last - 1, last - 1, 7]] * 3, EOT, BEG)  # one tick left against the text
    run(eng, z, [[]] * 3, EOT, BEG, mit=1500)
    run(eng, z, [[]] * 3, EOT, BEG, mit=-1)


@pytest.mark.parametrize("B", [1, 3, 64])
def test_rows_are_independent(eng, B):
    """The same bits for a row alone and as row 2 of 3 (and of 64): token, L and M."""
    V, EOT, BEG = 51865, 50257, 50364
    rng = np.random.default_rng(5)
    row = rand(rng, 1, V, 3.0)
    row[0, BEG:] += 4.0
    g = [BEG + 3, 17]
    t1, L1, M1 = run(eng, row, [g], EOT, BEG)
    z = rand(rng, max(B, 3), V, 3.0)
    z[2] = row[0]
    tB, LB, MB = run(eng, z, [g] * z.shape[0], EOT, BEG)
    assert tB[2] == t1[0] and LB[2].tobytes() == L1[0].tobytes() and MB[2].tobytes() == M1[0].tobytes()
    # rows of different lengths in one call: runs of equal length are launched together
    gens = [[], [BEG + 1], [BEG + 3, 17]] + [[BEG + 3, 17]] * (z.shape[0] - 3)
    tM, LM, _ = run(eng, z, gens, EOT, BEG)
    assert tM[2] == t1[0] and LM[2].tobytes() == L1[0].tobytes()


def test_logsumexp_accuracy(eng):
    V, EOT, BEG = 51865, 50257, 50364
    rng = np.random.default_rng(7)
    worst = 0.0
    for scale, shift in ((1.0, 0.0), (1.0, 40.0), (30.0, 0.0), (300.0, -100.0)):
        z = rand(rng, 8, V, scale) + np.float32(shift)
        for g in ([BEG, 3], [BEG + 700, 3], [BEG, 3, BEG + 1400]):
            tok, L, _ = eng.dbg_timestamp_select(z, np.array([[1, 1] + g + [0]] * 8, np.int64),
                                                 np.full(8, 2 + len(g), np.int32), SB, EOT, BEG, 50)
            for b in range(8):
                want = ts_ref.step(z[b], g, EOT, BEG)[1]["L"]
                worst = max(worst, abs(L[b] - want))
    print("largest |L - float64 L|: %.3e" % worst)
    assert worst <= L_BOUND
