"""GPU (-m gpu): sample_partial + sample_select of csrc/k_sample.hip (option temperature) through
the debug tap wt_dbg_sample_select, one step per row, against tests/sample_ref.py on the same fp32 logits: the whole
vocabulary and every state of the timestamp rules, eot / beg at, before and behind a chunk boundary, rule 5 both ways,
logits at scales 1, 30 and 300 and with -inf, temperatures 0.2, 0.6, 1.0 and 0 mixed in, winners at chunk edges, row
independence, the four counter words, and T = 0 against ts_select bit for bit.

Token equality is demanded wherever the reference's gap between the best and the second-best key exceeds the bar
sample_ref.key_bar derives from the arithmetic (one fmaf rounding, logf within 2 ulp through both logarithms); the seeds
were chosen on the CPU so that no row of any case lies under it, and a case tolerates at most one row in 64 there.
T = 0 rows are exact: they must equal the reference always."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sample_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

SB = 2  # sample_begin of every row here: a two-id prompt
worst = {"key": 0.0, "ratio": 0.0}  # largest |kernel key - float64 key|, and the largest such error over its bound


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def id_rows(gens):
    B = len(gens)
    ids = np.zeros((B, SB + max(len(g) for g in gens) + 1), np.int64)
    ids[:, :SB] = 1
    n = np.zeros(B, np.int32)
    for b, g in enumerate(gens):
        ids[b, SB:SB + len(g)] = g
        n[b] = SB + len(g)
    return ids, n


def run(eng, z, gens, temps, ts, eot, beg, mit=50, seed=0, attempt=0, clip_base=0, pos=-1):
    """One step per row, checked against sample_ref.step; returns (tokens, L, M, keys)."""
    z = np.ascontiguousarray(z, np.float32)
    B = z.shape[0]
    temps = np.broadcast_to(np.asarray(temps, np.float32), (B,))
    ids, n = id_rows(gens)
    tok, L, M, key = eng.dbg_sample_select(z, ids, n, SB, temps, seed, attempt, clip_base, pos, ts, eot, beg, mit)
    under = 0
    for b, g in enumerate(gens):
        p = pos if pos >= 0 else SB + len(g) - 1
        want, info = sr.step(z[b], list(g), temps[b], seed, p, clip_base + b, attempt, eot, beg, mit, ts)
        if temps[b] != 0 and not info["gap"] > info["bar"]:
            under += 1
            continue
        assert int(tok[b]) == want, (b, int(tok[b]), want, info)
        if np.isfinite(info["key"]):
            err = abs(float(key[b]) - info["key"])
            assert err <= info["key_bar"], (b, err, info)
            worst["key"] = max(worst["key"], err)
            if info["key_bar"] > 0:
                worst["ratio"] = max(worst["ratio"], err / info["key_bar"])
        else:
            assert float(key[b]) == info["key"]
        if ts:
            if info["L"] is None:
                assert np.isnan(L[b])
            elif info["L"] == -np.inf:
                assert L[b] == -np.inf
            else:
                assert abs(L[b] - info["L"]) <= 5e-7  # section 14's bound on rule 5's logsumexp
            assert np.isnan(M[b]) if info["M"] is None else M[b] == np.float32(info["M"])
        else:
            assert np.isnan(L[b]) and M[b] == np.float32(info["M"])
    assert under * 64 <= B, (under, B)
    return tok, L, M, key


def rand(rng, B, V, scale=1.0):
    return (rng.standard_normal((B, V)) * scale).astype(np.float32)


def mixed(B):
    """Temperatures of a batch that holds clips at 0 beside sampling ones."""
    return np.array([(0.0, 0.6, 0.2, 1.0)[b % 4] for b in range(B)], np.float32)


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("V", [4101, 8192, 51865])
def test_rows_equal_the_reference(eng, V, B):
    """Plain and timestamp mode at every temperature and logit scale, rows with -inf, a mixed batch."""
    rng = np.random.default_rng(1000 * B + V)
    beg = V - 1501 if V > 8192 else V - 101
    eot = beg - 107 if V > 8192 else beg - 7
    cases = [(0.2, 1.0, False), (0.6, 30.0, False), (1.0, 300.0, False), (None, 1.0, True)]
    for c, (T, scale, inf) in enumerate(cases):
        z = rand(rng, B, V, scale)
        if inf:
            z[:, rng.integers(0, V, V // 3)] = -np.inf  # -inf scattered over text and timestamps
        temps = mixed(B) if T is None else T
        run(eng, z, [[]] * B, temps, False, eot, beg, seed=c + 1, clip_base=c)
        z[:, beg:] += np.float32((2.0, -2.0, 6.0, 2.0)[c] * scale)  # rule 5 fires in some cases and rows, not in others
        g = ([beg + 3, 17], [beg + 1, 3, beg + 4, beg + 4, 9], [], [5])[c]
        run(eng, z, [g] * B, temps, True, eot, beg, seed=c + 1, attempt=c, clip_base=7)


@pytest.mark.parametrize("V", [4101, 8192, 51865])
def test_rule_states_and_chunk_boundaries(eng, V):
    """eot and beg at, before and behind a chunk boundary; an empty timestamp interval ([t]), text shrunk to {eot}
    ([t, 3, t']), a one-id timestamp interval (beg = V - 1, or the last tick reached), 0, 1, 2 and more generated ids;
    the timestamp logits raised or lowered so that rule 5 goes both ways."""
    rng = np.random.default_rng(V)
    edges = [4096] if V == 4101 else ([4096, 8190] if V == 8192 else [4096, 49152, 50364])
    temps3 = np.array([0.2, 0.6, 1.0], np.float32)
    fired = set()
    for edge in edges:
        for beg in (edge - 1, edge, edge + 1):
            for eot in (beg - 1, beg - 3, 4095 if beg > 4100 else 1):
                z = rand(rng, 3, V)
                z[:, beg:] += np.float32(rng.choice([-2.0, 2.0, 6.0]))
                t = [min(beg + d, V - 1) for d in (0, 1, 2, 3)]
                mit = int(rng.choice([-1, 0, 1, 50]))
                for g in ([], [t[0]], [3], [t[1], t[1]], [t[0], 3], [3, t[1]], [t[0], 3, t[2]], [t[0], 3, t[2], t[2], 4],
                          [t[0], 3, V - 1], [t[0], 3, V - 2, V - 2, 4]):
                    _, L, M, _ = run(eng, z, [g] * 3, temps3, True, eot, beg, mit, seed=edge + beg)
                    if not np.isnan(L[0]) and not np.isnan(M[0]):
                        fired.add(bool(L[0] > M[0]))
    assert fired == {True, False}
    z = rand(rng, 3, V)
    for g in ([], [V - 1], [V - 1, V - 1], [V - 1, 7], [V - 1, 7, V - 1]):
        run(eng, z, [g] * 3, temps3, True, V - 3, V - 1)  # one timestamp: beg = V - 1
    for g in ([], [5], [5, 5], [5, 0], [5, 0, 9]):
        run(eng, z, [g] * 3, temps3, True, 0, 1)          # text is EOT alone: eot = 0, beg = 1


def test_winners_at_chunk_edges(eng):
    """A logit far above the rest at the first and the last entry of a chunk, at id 0 and at V - 1: the sample is that id."""
    rng = np.random.default_rng(3)
    for V in (4101, 8192, 51865):
        spots = [0, 4095, 4096, V - 1] + ([8191] if V >= 8192 else []) + ([49151, 49152] if V > 50000 else [])
        z = rand(rng, len(spots), V)
        for b, i in enumerate(spots):
            z[b, i] = 100.0  # the noise spans 19.5: the key of this id wins at every temperature up to 1
        for T in (0.2, 1.0):
            tok, _, _, _ = run(eng, z, [[]] * len(spots), T, False, 1, 2, seed=9)
            assert [int(x) for x in tok] == spots


@pytest.mark.parametrize("B", [1, 3, 64])
def test_rows_are_independent(eng, B):
    """The same bits for a row alone and as row 2 of 3 (and of 64) under the same clip index: token, key, L and M."""
    V, EOT, BEG = 51865, 50257, 50364
    rng = np.random.default_rng(5)
    row = rand(rng, 1, V, 3.0)
    row[0, BEG:] += 4.0
    g = [BEG + 3, 17]
    for ts in (False, True):
        one = run(eng, row, [g], 0.6, ts, EOT, BEG, seed=11, attempt=2, clip_base=2)
        z = rand(rng, max(B, 3), V, 3.0)
        z[2] = row[0]
        many = run(eng, z, [g] * z.shape[0], 0.6, ts, EOT, BEG, seed=11, attempt=2, clip_base=0)
        for a, b in zip(one, many):
            assert a[0].tobytes() == b[2].tobytes()
        # rows of different lengths in one call (runs of equal length are launched together), the position given
        gens = [[], [BEG + 1], g] + [g] * (z.shape[0] - 3)
        p = SB + len(g) - 1
        diff = run(eng, z, gens, 0.6, ts, EOT, BEG, seed=11, attempt=2, clip_base=0, pos=p)
        assert diff[0][2] == one[0][0] and diff[3][2].tobytes() == one[3][0].tobytes()


def test_every_counter_word_and_the_seed_matter(eng):
    """64 rows of ONE logits row: the clip index alone makes them differ, and so does each of seed, attempt and pos
    (every run is also checked against the reference under those values)."""
    V, EOT, BEG = 4101, 3000, 3990
    rng = np.random.default_rng(6)
    z = np.repeat(rand(rng, 1, V), 64, axis=0)
    base = dict(seed=(5 << 32) | 3, attempt=1, clip_base=0, pos=9)
    t0 = run(eng, z, [[]] * 64, 1.0, False, EOT, BEG, **base)[0]
    assert np.unique(t0).size > 32  # the rows differ by their clip index alone
    for change in (dict(seed=(5 << 32) | 4), dict(seed=(6 << 32) | 3), dict(attempt=2), dict(pos=10), dict(clip_base=64)):
        t1 = run(eng, z, [[]] * 64, 1.0, False, EOT, BEG, **dict(base, **change))[0]
        assert (t1 != t0).any(), change
    same = run(eng, z, [[]] * 64, 1.0, False, EOT, BEG, **base)[0]
    assert np.array_equal(same, t0)


def test_zero_temperature_is_ts_select_bit_for_bit(eng):
    """T = 0 rows: token, L and M of wt_dbg_timestamp_select, bit for bit; L and M are those at every temperature."""
    V, EOT, BEG = 51865, 50257, 50364
    rng = np.random.default_rng(7)
    for scale, shift in ((1.0, 2.0), (30.0, 0.0), (300.0, -100.0)):
        z = rand(rng, 64, V, scale)
        z[:, BEG:] += np.float32(shift)
        z[1] = np.round(z[1])  # many exact ties: the larger id
        z[2, rng.integers(0, V, 20000)] = -np.inf
        for g in ([], [BEG + 3, 17], [BEG, 3, BEG + 1400], [BEG + 2]):
            ids, n = id_rows([g] * 64)
            tok, L, M = eng.dbg_timestamp_select(z, ids, n, SB, EOT, BEG, 50)
            t0, L0, M0, k0 = eng.dbg_sample_select(z, ids, n, SB, 0.0, 3, 1, 0, -1, True, EOT, BEG, 50)
            assert np.array_equal(t0, tok) and L0.tobytes() == L.tobytes() and M0.tobytes() == M.tobytes()
            assert np.array_equal(k0, z[np.arange(64), tok])  # the key is the logit itself
            for T in (0.2, 1.0):
                _, L1, M1, _ = eng.dbg_sample_select(z, ids, n, SB, T, 3, 1, 0, -1, True, EOT, BEG, 50)
                assert L1.tobytes() == L.tobytes() and M1.tobytes() == M.tobytes()
    # plain mode at T = 0: the last maximal id of the row
    z = rand(rng, 64, V)
    z[1] = np.round(z[1])
    ids, n = id_rows([[]] * 64)
    t0 = eng.dbg_sample_select(z, ids, n, SB, 0.0, 3, 1, 0, -1, False, EOT, BEG, 50)[0]
    assert [int(t) for t in t0] == [int(np.flatnonzero(r == r.max())[-1]) for r in z]


def test_refused_arguments(eng, pkg):
    z = np.zeros((2, 4101), np.float32)
    ids, n = id_rows([[]] * 2)
    bad = [dict(temperature=-0.5), dict(temperature=np.inf), dict(attempt=-1), dict(clip_base=-1),
           dict(timestamps=True, eot=4000, beg=4000), dict(timestamps=True, eot=10, beg=4101), dict(eot=4101)]
    for kw in bad:
        args = dict(temperature=0.6, seed=0, attempt=0, clip_base=0, pos=-1, timestamps=False, eot=10, beg=20)
        args.update(kw)
        with pytest.raises(pkg.WtError) as e:
            eng.dbg_sample_select(z, ids, n, SB, **args)
        assert str(e.value).startswith("WT_ERR_INVALID_ARG"), kw
    with pytest.raises(pkg.WtError) as e:  # sample_begin below 1
        eng.dbg_sample_select(z[:, :4101], np.zeros((2, 2), np.int64), np.zeros(2, np.int32), 0, 0.6)
    assert str(e.value).startswith("WT_ERR_INVALID_ARG")
    many = np.zeros((65, 4101), np.float32)  # more than 64 rows
    ids65, n65 = id_rows([[]] * 65)
    with pytest.raises(pkg.WtError) as e:
        eng.dbg_sample_select(many, ids65, n65, SB, 0.6)
    assert str(e.value).startswith("WT_ERR_INVALID_ARG")
    eng.dbg_sample_select(z, ids, n, SB, 0.6)  # the engine stays usable


def test_zz_report():
    print("largest |kernel key - float64 key|: %.3e; largest error over its bound: %.3f" % (worst["key"], worst["ratio"]))
