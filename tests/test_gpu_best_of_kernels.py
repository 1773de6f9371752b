"""GPU (-m gpu): the kernels behind several samples per clip through their debug taps.

The grouped sampler (k_sample.hip, SampleArgs::group; wt_dbg_sample_select_group) against tests/sample_ref.step on the
same fp32 logits: row r of a launch over `clips` clips is sample j = r // clips of clip c = r % clips and must be the
reference's step under the clip word clip_base + row0 + c, the attempt word attempt + (j << 16) and the clip's own
temperature.  Token equality is demanded wherever the reference's gap between the best and the second-best key exceeds
the bar sample_ref.key_bar derives from the arithmetic, as tests/test_gpu_sample_kernel.py demands it; a case tolerates
at most one row in 64 under the bar, T = 0 rows none.  Sample 0, and every row of group = 1, equal wt_dbg_sample_select
bit for bit.

best_of_begin and best_of_pick (k_best_of.hip) against tests/best_of_ref.py, exactly: they move ids and float64 sums and
compare float64 quotients, so every output bit is determined."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import best_of_ref as bo  # noqa: E402
import sample_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

SB = 2  # sample_begin of every row here: a two-id prompt


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def id_rows(g, B):
    ids = np.zeros((B, SB + len(g) + 1), np.int64)
    ids[:, :SB] = 1
    ids[:, SB:SB + len(g)] = g
    return ids, SB + len(g)


def clip_temps(clips):
    """Clips at T = 0 beside sampled ones."""
    return np.array([(0.6, 0.0, 0.2, 1.0)[c % 4] for c in range(clips)], np.float32)


def run(eng, z, g, temps, N, ts, eot, beg, mit=50, seed=0, attempt=0, clip_base=0, row0=0, pos=-1):
    """One grouped launch, every row checked against sample_ref.step; returns (tokens, L, M, keys)."""
    z = np.ascontiguousarray(z, np.float32)
    B = z.shape[0]
    clips = (B + N - 1) // N
    temps = np.broadcast_to(np.asarray(temps, np.float32), (clips,))
    ids, n = id_rows(g, B)
    tok, L, M, key = eng.dbg_sample_select_group(z, ids, n, SB, temps, N, seed, attempt, clip_base, row0, pos, ts, eot, beg, mit)
    under = 0
    for r in range(B):
        c, j = r % clips, r // clips
        p = pos if pos >= 0 else n - 1
        want, info = sr.step(z[r], list(g), temps[c], seed, p, clip_base + row0 + c, bo.attempt_word(attempt, j), eot, beg,
                             mit, ts)
        if temps[c] != 0 and not info["gap"] > info["bar"]:
            under += 1
            continue
        assert int(tok[r]) == want, (r, c, j, int(tok[r]), want, info)
        if np.isfinite(info["key"]):
            assert abs(float(key[r]) - info["key"]) <= info["key_bar"], (r, info)
        else:
            assert float(key[r]) == info["key"]
        if ts:
            if info["L"] is None:
                assert np.isnan(L[r])
            elif info["L"] == -np.inf:
                assert L[r] == -np.inf
            else:
                assert abs(L[r] - info["L"]) <= 5e-7  # section 14's bound on rule 5's logsumexp
            assert np.isnan(M[r]) if info["M"] is None else M[r] == np.float32(info["M"])
        else:
            assert np.isnan(L[r]) and M[r] == np.float32(info["M"])
    assert under * 64 <= B, (under, B)
    return tok, L, M, key


def rand(rng, B, V, scale=1.0):
    return (rng.standard_normal((B, V)) * scale).astype(np.float32)


def vocab_ids(V):
    beg = V - 1501 if V > 8192 else V - 101
    return (beg - 107 if V > 8192 else beg - 7), beg


@pytest.mark.parametrize("N", [1, 2, 5, 8])
@pytest.mark.parametrize("V", [4101, 8192, 51865])
def test_rows_equal_the_reference(eng, V, N):
    """1, N and 128 rows (N = 1: 64, the parameter block's clips; N = 5: 128 rows are 26 clips, of which the last sample
    has no rows for clips 24 and 25); plain and timestamp mode, rows with -inf, rule 5 firing in some rows and not in
    others, clips at T = 0 beside sampled ones, a non-zero attempt, clip base and first clip."""
    rng = np.random.default_rng(100 * V + N)
    eot, beg = vocab_ids(V)
    fired = set()
    for k, B in enumerate((1, N, 128 if N > 1 else 64)):
        clips = (B + N - 1) // N
        temps = clip_temps(clips) if clips > 1 else (0.2, 1.0, 0.6)[k]
        scale = (1.0, 30.0, 1.0)[k]
        z = rand(rng, B, V, scale)
        z[B // 2, rng.integers(0, V, V // 3)] = -np.inf  # -inf scattered over text and timestamps
        run(eng, z, [], temps, N, False, eot, beg, seed=k + 1, attempt=k, clip_base=3 * k, row0=0 if clips > 60 else k)
        # (1501 timestamps of unit variance have a logsumexp near 7.8 and the best text logit is near 4.3: -8 keeps rule 5 off)
        z[:, beg:] += (rng.choice([-8.0, 2.0, 6.0], (B, 1)) * scale).astype(np.float32)
        g = ([beg + 3, 17], [], [beg + 1, 3, beg + 4, beg + 4, 9])[k]
        _, L, M, _ = run(eng, z, g, temps, N, True, eot, beg, seed=(k + 1) << 33 | 5, attempt=k, clip_base=7)
        fired |= {bool(a > b) for a, b in zip(L, M) if not np.isnan(a) and not np.isnan(b)}
    assert fired == {True, False}


@pytest.mark.parametrize("N", [2, 5, 8])
def test_sample_zero_is_the_ungrouped_draw(eng, N):
    """The rows j = 0 of a grouped launch equal wt_dbg_sample_select on the same rows bit for bit (token, key, L, M)."""
    V = 51865
    eot, beg = vocab_ids(V)
    rng = np.random.default_rng(N)
    clips = 128 // N
    B = N * clips
    z = rand(rng, B, V, 3.0)
    z[:, beg:] += 4.0
    temps = clip_temps(clips)
    g = [beg + 3, 17]
    for ts in (False, True):
        ids, n = id_rows(g, B)
        grouped = eng.dbg_sample_select_group(z, ids, n, SB, temps, N, 11, 2, 5, 0, -1, ts, eot, beg, 50)
        plain = eng.dbg_sample_select(z[:clips], ids[:clips], np.full(clips, n, np.int32), SB, temps, 11, 2, 5, -1, ts, eot, beg, 50)
        for a, b in zip(grouped, plain):
            assert a[:clips].tobytes() == b.tobytes()


def test_group_of_one_is_the_ungrouped_launch(eng):
    V = 8192
    eot, beg = vocab_ids(V)
    rng = np.random.default_rng(4)
    z = rand(rng, 64, V, 3.0)
    temps = clip_temps(64)
    ids, n = id_rows([beg + 2], 64)
    for ts in (False, True):
        grouped = eng.dbg_sample_select_group(z, ids, n, SB, temps, 1, 9, 1, 2, 0, 7, ts, eot, beg, 50)
        plain = eng.dbg_sample_select(z, ids, np.full(64, n, np.int32), SB, temps, 9, 1, 2, 7, ts, eot, beg, 50)
        for a, b in zip(grouped, plain):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N", [2, 5, 8])
def test_a_row_alone_and_among_128(eng, N):
    """Row r = j * clips + c of a full launch gives the bits of the same logits row launched alone under the words the
    grouped kernel forms for it: clip word clip_base + c, attempt word attempt + (j << 16)."""
    V = 51865
    eot, beg = vocab_ids(V)
    rng = np.random.default_rng(50 + N)
    clips = (128 + N - 1) // N
    z = rand(rng, 128, V, 3.0)
    z[:, beg:] += 4.0
    g = [beg + 3, 17]
    ids, n = id_rows(g, 128)
    for ts in (False, True):
        full = eng.dbg_sample_select_group(z, ids, n, SB, 0.6, N, 11, 2, 4, 0, -1, ts, eot, beg, 50)
        for r in (0, clips - 1, clips, 127):
            c, j = r % clips, r // clips
            one = eng.dbg_sample_select(z[r:r + 1], ids[:1], np.full(1, n, np.int32), SB, 0.6, 11, bo.attempt_word(2, j), 4 + c, -1,
                                        ts, eot, beg, 50)
            for a, b in zip(full, one):
                assert a[r:r + 1].tobytes() == b.tobytes(), (r, c, j)


def test_samples_of_a_clip_differ(eng):
    """8 samples of 16 clips over ONE logits row: the sample index alone makes a clip's rows differ, the clip index alone
    the rows of a sample; the same launch again gives the same tokens."""
    V, eot, beg = 4101, 3000, 3990
    z = np.repeat(rand(np.random.default_rng(6), 1, V), 128, axis=0)
    tok, _, _, key = run(eng, z, [], 1.0, 8, False, eot, beg, seed=(5 << 32) | 3, attempt=1, pos=9)
    tok, key = tok.reshape(8, 16), key.reshape(8, 16)
    for c in range(16):
        assert np.unique(key[:, c]).size == 8, c
    for j in range(8):
        assert np.unique(key[j]).size == 16, j
    assert np.unique(tok).size > 64
    again = run(eng, z, [], 1.0, 8, False, eot, beg, seed=(5 << 32) | 3, attempt=1, pos=9)[0]
    assert np.array_equal(again.reshape(8, 16), tok)


def test_sampler_refusals(eng, pkg):
    V = 4101
    z = np.zeros((130, V), np.float32)
    ids, n = id_rows([], 130)
    ok = dict(seed=0, attempt=0, clip_base=0, row0=0, pos=-1, timestamps=False, eot=10, beg=20)
    bad = [(128, 9, {}), (128, 0, {}), (130, 2, {}), (65, 1, {}), (128, 2, dict(row0=1)), (10, 5, dict(row0=63)),
           (10, 5, dict(row0=-1)), (10, 5, dict(attempt=-1)), (10, 5, dict(eot=V)), (10, 5, dict(timestamps=True, eot=30, beg=20))]
    for B, N, kw in bad:
        with pytest.raises(pkg.WtError) as e:
            eng.dbg_sample_select_group(z[:B], ids[:B], n, SB, 0.6, N, **dict(ok, **kw))
        assert str(e.value).startswith("WT_ERR_INVALID_ARG"), (B, N, kw)
    with pytest.raises(pkg.WtError) as e:
        eng.dbg_sample_select_group(z[:10], ids[:10], n, SB, -1.0, 5, **ok)
    assert str(e.value).startswith("WT_ERR_INVALID_ARG")
    eng.dbg_sample_select_group(z[:128], ids[:128], n, SB, 0.6, 2, **ok)  # the engine stays usable
    eng.dbg_sample_select_group(z[:10], ids[:10], n, SB, 0.6, 5, **dict(ok, row0=62))


# ---- k_best_of.hip ----
@pytest.mark.parametrize("N", [1, 2, 3, 5, 8])
def test_begin_rows_and_table(eng, N):
    rng = np.random.default_rng(N)
    for clips, n_prompt, cap in ((1, 1, 40), (128 // N if N > 1 else 64, 4, 448), (3, 2, 40), (2, 40, 40)):
        stride = cap + 1
        prompts = rng.integers(1, 50000, (clips, stride))
        frozen = None if clips == 3 else (rng.random(clips) < 0.4).astype(np.int32)
        ids = np.full((N * clips, stride), 12345, np.int64)
        ids[:clips] = prompts
        got = eng.dbg_best_of_begin(ids, n_prompt, N, cap, frozen)
        want = bo.begin(prompts, n_prompt, N, cap, frozen)
        for name, a, b in zip(("ids", "n_ids", "finished", "sum", "count", "anc"), got, want):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, clips, n_prompt)


def pick_case(rng, N, clips, stride, special):
    R = N * clips
    ids = rng.integers(1, 50000, (R, stride))
    lp = -rng.random((R, stride)).astype(np.float32) * 3
    n_ids = rng.integers(3, stride + 1, R).astype(np.int32)
    counts = (n_ids - 2).astype(np.int32)
    sums = np.array([lp[r, 2:n_ids[r]].astype(np.float64).sum() for r in range(R)])
    if special:  # ties, +-0, -inf sums, NaNs, counts of 1 and 0, ids counts outside the row
        for c in range(clips):
            rows = [j * clips + c for j in range(N)]
            kind = c % 8
            if kind == 0:
                sums[rows], counts[rows] = -2.0 * np.arange(1, N + 1), np.arange(1, N + 1)       # all equal: the first
            elif kind == 1:
                sums[rows], counts[rows] = [(-0.0, 0.0)[j % 2] for j in range(N)], 1
            elif kind == 2:
                sums[rows[::2]] = -np.inf
            elif kind == 3:
                sums[rows] = -np.inf
            elif kind == 4:
                sums[rows[0]] = np.nan
            elif kind == 5:
                sums[rows] = np.nan
            elif kind == 6:
                counts[rows[0]], counts[rows[-1]] = 0, 1
                sums[rows[0]] = 0.0
            else:
                n_ids[rows[0]], n_ids[rows[-1]] = stride + 5, -3
                if N > 1:
                    sums[rows[-1]], counts[rows[-1]] = sums[rows[0]] * 2, counts[rows[0]] * 2    # a tie of first and last
    return ids, lp, n_ids, sums, counts


def pick_out(rng, n_out, stride):
    return {"ids": rng.integers(1, 99, (n_out, stride)), "lp": rng.random((n_out, stride)).astype(np.float32),
            "n": rng.integers(1, 99, n_out).astype(np.int32), "count": rng.integers(1, 99, n_out).astype(np.int32),
            "picked": rng.integers(10, 99, n_out).astype(np.int32), "sum": rng.random(n_out),
            "all_sum": rng.random((n_out, 8)), "all_count": rng.integers(1, 99, (n_out, 8)).astype(np.int32)}


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6, 7, 8])
def test_pick_equals_numpy(eng, N):
    """Random rows and the special ones at 1, 2, 9 and the most clips a chain of N has, strides 41 and 449, the chain's
    first output row at 0, in the middle and at the end of the 64; the other output rows keep their bytes."""
    rng = np.random.default_rng(70 + N)
    most = min(128 // N, 64)
    for clips in sorted({1, 2, min(9, most), most}):
        for stride in (41, 449):
            for special in (False, True):
                n_out = (64, clips, clips + 3)[(clips + stride + special) % 3]
                c0 = (n_out - clips, 0, (n_out - clips) // 2)[(clips + special) % 3]
                case = pick_case(rng, N, clips, stride, special)
                out = pick_out(rng, n_out, stride)
                got = eng.dbg_best_of_pick(*case, N, c0, out)
                want = bo.pick(*case, N, c0, out)
                for k in want:
                    assert got[k].tobytes() == want[k].tobytes(), (k, clips, stride, special, c0, n_out)
                inside = np.zeros(n_out, bool)
                inside[c0:c0 + clips] = True
                assert all(got[k][~inside].tobytes() == np.asarray(out[k])[~inside].tobytes() for k in out)


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6, 7, 8])
def test_pick_at_every_clip_count(eng, N):
    """Every clip count a chain of N samples can have, 1 .. min(128 / N, 64), at stride 41 with the special rows."""
    rng = np.random.default_rng(170 + N)
    for clips in range(1, min(128 // N, 64) + 1):
        c0 = (64 - clips, 0, (64 - clips) // 2)[clips % 3]
        case = pick_case(rng, N, clips, 41, True)
        out = pick_out(rng, 64, 41)
        got = eng.dbg_best_of_pick(*case, N, c0, out)
        want = bo.pick(*case, N, c0, out)  # (rows outside c0 .. c0 + clips keep their bytes in it)
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), (k, clips, c0)


def test_best_of_refusals(eng, pkg):
    rng = np.random.default_rng(1)
    for N, clips, stride, c0, n_out in ((9, 2, 41, 0, 64), (5, 26, 41, 0, 64), (2, 4, 41, 61, 64), (2, 4, 41, -1, 64),
                                        (2, 4, 450, 0, 64), (2, 4, 1, 0, 64), (2, 4, 41, 0, 3), (2, 4, 41, 0, 65)):
        ids, lp, n_ids, sums, counts = pick_case(rng, N, clips, max(stride, 4), False)
        ids, lp = ids[:, :stride], lp[:, :stride]
        with pytest.raises(pkg.WtError) as e:
            eng.dbg_best_of_pick(ids, lp, n_ids, sums, counts, N, c0, pick_out(rng, n_out, stride))
        assert str(e.value).startswith("WT_ERR_INVALID_ARG"), (N, clips, stride, c0, n_out)
    for N, clips, n_prompt, cap in ((9, 2, 2, 40), (5, 26, 2, 40), (2, 65, 2, 40), (2, 4, 0, 40), (2, 4, 41, 40), (2, 4, 2, 449)):
        with pytest.raises(pkg.WtError) as e:
            eng.dbg_best_of_begin(np.ones((N * clips, cap + 1), np.int64), n_prompt, N, cap)
        assert str(e.value).startswith("WT_ERR_INVALID_ARG"), (N, clips, n_prompt, cap)
    eng.dbg_best_of_begin(np.ones((8, 41), np.int64), 2, 2, 40)  # the engine stays usable

