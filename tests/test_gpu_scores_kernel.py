"""GPU (-m gpu): score_partial + score_finish of csrc/k_scores.hip (option scores) through the debug
tap wt_dbg_token_scores, one step per row, against tests/scores_ref.py (float64 numpy on the same fp32 logits): the whole
vocabulary and the intervals of the timestamp rules, eot / beg at, before and behind a 4096-entry chunk boundary, rule 5
firing and not, chosen ids at chunk edges, rows with -inf and allowed sets that are all -inf, the carried sum and count of
live and finished clips, 1, 3 and 64 rows, and row independence."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scores_ref as sr  # noqa: E402
import ts_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SB = 2  # sample_begin of every row here: a two-id prompt
# The device forms lp = fp32(z[tok] - D) with D the float64 merge of fp32 chunk sums, so |lp - lp64| <= |D - D64| +
# |lp| 2^-24.  Measured over the tables of this file on an MI355X (test_accuracy prints both): largest |D - D64| =
# MEASURED_DEN, largest |lp - lp64| = MEASURED_LP (half an fp32 ulp of an lp between 8 and 16; the rows spread by 300
# have lp near -1e3, but there the top logit IS the log-sum-exp and z - D is exact in fp32).  The bound on the
# denominator is five times the measured error (DESIGN.md section 14's convention), below the 2.7e-6 worst case of the
# chunk sums (expf within 2 ulp, the rounded argument, at most 24 additions per path); lp adds its own fp32 rounding.
MEASURED_DEN, MEASURED_LP = 1.341e-7, 9.54e-7
DEN_BOUND = 5 * MEASURED_DEN  # 6.7e-7
assert DEN_BOUND < 2.7e-6
worst = {"den": 0.0, "lp": 0.0}


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def rand(rng, B, V, scale=1.0):
    return (rng.standard_normal((B, V)) * scale).astype(np.float32)


def run(eng, z, toks, gens=None, ts=False, eot=0, beg=1, mit=50, live=None, sums=None, counts=None):
    """One step per row: logits z [B][V], the chosen id toks[b] behind the generated ids gens[b] and the prompt [1, 1].
    Checks lp, denominator, sum and count of every row against scores_ref and returns the tap's (lp, sums, counts, den)."""
    z = np.ascontiguousarray(z, np.float32)
    B = z.shape[0]
    gens = [[]] * B if gens is None else gens
    stride = SB + max(len(g) for g in gens) + 1
    ids = np.zeros((B, stride), np.int64)
    ids[:, :SB] = 1
    n = np.zeros(B, np.int32)
    for b, g in enumerate(gens):
        ids[b, SB:SB + len(g)] = g
        ids[b, SB + len(g)] = toks[b]
        n[b] = SB + len(g) + 1
    live = np.ones(B, np.int32) if live is None else np.asarray(live, np.int32)
    s0 = np.zeros(B) if sums is None else np.asarray(sums, np.float64)
    c0 = np.zeros(B, np.int32) if counts is None else np.asarray(counts, np.int32)
    lp, s1, c1, den = eng.dbg_token_scores(z, ids, n, SB, live, s0, c0, ts, eot, beg, mit)
    for b, g in enumerate(gens):
        want, dwant = sr.token_logprob(z[b], int(toks[b]), list(g), eot, beg, mit, ts)
        if dwant == -math.inf:
            assert den[b] == -math.inf and lp[b] == -math.inf, (b, den[b], lp[b])
        else:
            worst["den"] = max(worst["den"], abs(den[b] - dwant))
            assert abs(den[b] - dwant) <= DEN_BOUND, (b, den[b], dwant)
            if want == -math.inf:
                assert lp[b] == -math.inf
            else:
                worst["lp"] = max(worst["lp"], abs(lp[b] - want))
                assert abs(lp[b] - want) <= DEN_BOUND + abs(want) * 2.0 ** -24 * 1.001, (b, lp[b], want)
        assert not np.isnan(lp[b]) and not np.isnan(den[b])
        if live[b]:  # the device adds the fp32 lp it wrote, in float64
            assert c1[b] == c0[b] + 1 and (s1[b] == s0[b] + np.float64(lp[b]) or (np.isinf(lp[b]) and s1[b] == -math.inf))
        else:
            assert c1[b] == c0[b] and s1[b] == s0[b]
    return lp, s1, c1, den


@pytest.mark.parametrize("V", [4101, 8192, 51865])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_whole_vocabulary_and_chosen_ids_at_chunk_edges(eng, V, B):
    rng = np.random.default_rng(V + B)
    z = rand(rng, B, V, 2.0)
    last_chunk = (V - 1) // 4096 * 4096
    for tok in (0, 4095, 4096, last_chunk, V - 1):  # first / last entry of a chunk, V - 1
        run(eng, z, [tok] * B)
    run(eng, z, rng.integers(0, V, B))


@pytest.mark.parametrize("V", [4101, 8192, 51865])
def test_intervals_at_chunk_boundaries_and_rule_5_both_ways(eng, V):
    """eot and beg at, before and behind a chunk boundary; every shape of the two intervals; the timestamp logits raised
    or lowered so that rule 5 fires and does not."""
    rng = np.random.default_rng(V)
    edges = [4096] if V == 4101 else ([4096, 8190] if V == 8192 else [4096, 49152, 50364])
    fired = set()
    for edge in edges:
        for beg in (edge - 1, edge, edge + 1):
            for eot in (beg - 1, beg - 3, 4095 if beg > 4100 else 1):
                z = rand(rng, 3, V)
                z[:, beg:] += np.float32(rng.choice([-2.0, 2.0, 6.0]))
                t = [min(beg + d, V - 1) for d in (0, 1, 2, 3)]
                # no timestamps (empty interval), text shrunk to {eot}, the first step, a one-id timestamp interval ...
                for g in ([], [t[0]], [3], [t[1], t[1]], [t[0], 3], [t[0], 3, t[2]], [t[0], 3, V - 1], [t[0], 3, V - 1, V - 1, 4]):
                    mit = int(rng.choice([-1, 0, 1, 50]))
                    tok, info = ts_ref.step(z[0], g, eot, beg, mit)
                    fired.add("mass" in info["fired"])
                    toks = [ts_ref.step(z[b], g, eot, beg, mit)[0] for b in range(3)]  # what ts_select would choose
                    run(eng, z, toks, [g] * 3, True, eot, beg, mit)
    assert fired == {True, False}


def test_one_id_intervals(eng):
    rng = np.random.default_rng(1)
    z = rand(rng, 3, 4101)
    for g, tok in (([], 4100), ([4100, 7], 7), ([4100, 7, 4100], 4098), ([4100, 7, 4100], 4100)):
        run(eng, z, [tok] * 3, [g] * 3, True, 4098, 4100)  # one timestamp: beg = V - 1; text {eot} behind a closed segment
    lp = run(eng, z, [0] * 3, [[5, 5]] * 3, True, 0, 1)[0]   # text is EOT alone (eot = 0, beg = 1) behind a pair
    assert (lp == 0.0).all()                                # one allowed id: probability 1


@pytest.mark.parametrize("scale,shift", [(1.0, 0.0), (1.0, 40.0), (30.0, 0.0), (300.0, -100.0)])
def test_accuracy_on_spread_logits(eng, scale, shift):
    V, EOT, BEG = 51865, 50257, 50364
    rng = np.random.default_rng(7)
    z = rand(rng, 8, V, scale) + np.float32(shift)
    run(eng, z, rng.integers(0, V, 8))
    run(eng, z, z.argmax(axis=1))
    for g in ([BEG, 3], [BEG + 700, 3], [BEG, 3, BEG + 1400], []):
        toks = [ts_ref.step(z[b], g, EOT, BEG)[0] for b in range(8)]
        run(eng, z, toks, [g] * 8, True, EOT, BEG)
    print("largest |D - D64|: %.3e, largest |lp - lp64|: %.3e (so far in this session)" % (worst["den"], worst["lp"]))


def test_minus_infinity(eng):
    V, EOT, BEG = 8192, 4090, 4097
    rng = np.random.default_rng(3)
    z = rand(rng, 3, V)
    z[:, rng.integers(0, V, 3000)] = -np.inf  # scattered over both intervals
    z[1, 7] = -np.inf
    run(eng, z, [7, 7, 8000])
    run(eng, z, [7, 7, BEG + 5], [[BEG + 1, 2]] * 3, True, EOT, BEG)
    z[:] = -np.inf  # the allowed set is all -inf: lp = -inf, no NaN
    lp, s, c, den = run(eng, z, [5, 5, 5], sums=[-1.5, 0.0, 2.0], counts=[3, 0, 1], live=[1, 0, 1])
    assert (lp == -np.inf).all() and (den == -np.inf).all() and s[1] == 0.0 and list(c) == [4, 0, 2]
    z = rand(rng, 3, V)
    z[:, BEG:] = -np.inf  # the timestamps alone are -inf: L = -inf is not above M, the text decides
    lp = run(eng, z, [3, 3, 3], [[BEG + 1, 2]] * 3, True, EOT, BEG)[0]
    assert np.isfinite(lp).all()
    z[:, :BEG] = -np.inf
    lp = run(eng, z, [3, 3, V - 1], [[BEG + 1, 2]] * 3, True, EOT, BEG)[0]
    assert (lp == -np.inf).all()


def test_carried_sum_and_count(eng):
    """A clip finished before the step adds nothing; a clip that finishes on this step adds its EOT."""
    V, EOT = 4101, 4000
    rng = np.random.default_rng(4)
    z = rand(rng, 3, V)
    z[1, EOT] = 9.0
    lp, s, c, _ = run(eng, z, [17, EOT, 17], live=[0, 1, 1], sums=[-3.25, -1.0, -0.5], counts=[7, 2, 1])
    assert s[0] == -3.25 and c[0] == 7                       # finished before: untouched, though lp is still written
    assert c[1] == 3 and s[1] == -1.0 + np.float64(lp[1])    # finishes here: the EOT counts
    assert c[2] == 2 and lp[0] < 0.0


@pytest.mark.parametrize("B", [3, 64])
def test_rows_are_independent(eng, B):
    """The same bits for a row alone and as row 2 of 3 (and of 64): lp and the denominator, plain and with timestamps."""
    V, EOT, BEG = 51865, 50257, 50364
    rng = np.random.default_rng(5)
    row = rand(rng, 1, V, 3.0)
    row[0, BEG:] += 4.0
    g = [BEG + 3, 17]
    z = rand(rng, B, V, 3.0)
    z[2] = row[0]
    for ts in (False, True):
        tok = ts_ref.step(row[0], g, EOT, BEG)[0] if ts else 12345
        l1, _, _, d1 = run(eng, row, [tok], [g], ts, EOT, BEG)
        lB, _, _, dB = run(eng, z, [tok] * B, [g] * B, ts, EOT, BEG)
        assert lB[2].tobytes() == l1[0].tobytes() and dB[2].tobytes() == d1[0].tobytes()
    # rows of different lengths in one call: runs of equal length are launched together
    gens = [[], [BEG + 1], g] + [g] * (B - 3)
    toks = [ts_ref.step(z[b], gens[b], EOT, BEG)[0] for b in range(B)]
    lM, _, _, dM = run(eng, z, toks, gens, True, EOT, BEG)
    l1, _, _, d1 = run(eng, row, [toks[2]], [g], True, EOT, BEG)
    assert lM[2].tobytes() == l1[0].tobytes() and dM[2].tobytes() == d1[0].tobytes()


def test_bad_arguments_are_refused(eng, pkg):
    z = np.zeros((1, 64), np.float32)
    ids = np.array([[1, 1, 5]], np.int64)
    for kw in ({"eot": 9, "beg": 9}, {"eot": 3, "beg": 64}):  # needs 0 <= eot < beg < V
        with pytest.raises(pkg.WtError):
            eng.dbg_token_scores(z, ids, np.array([3], np.int32), SB, timestamps=True, **kw)
    with pytest.raises(pkg.WtError):
        eng.dbg_token_scores(z, ids, np.array([2], np.int32), SB)  # no chosen id behind the prompt
    lp = eng.dbg_token_scores(z, np.array([[1, 1, 9999]], np.int64), np.array([3], np.int32), SB)[0]
    assert lp[0] == pytest.approx(-math.log(64.0), abs=1e-6)       # an id outside [0, V) is clamped before it indexes the row
