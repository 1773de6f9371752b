"""CPU: tests/best_of_ref.py (several samples per clip) on hand-made rows — the ranking rule, the
attempt word of sample j, the row layout and the two kernels' reference forms — and the exported debug taps."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import best_of_ref as bo  # noqa: E402
import sample_ref as sr  # noqa: E402


def test_ranking_first_best():
    assert bo.rank([-3.0, -2.0, -2.5], [3, 2, 5]) == 2          # averages -1, -1, -0.5
    assert bo.rank([-3.0, -2.0, -4.0], [3, 2, 4]) == 0          # all -1: the first
    assert bo.rank([-4.0, -2.0, -3.0], [2, 2, 3]) == 1          # -2, -1, -1: the first of the best two
    assert bo.rank([0.0, -0.0], [1, 1]) == 0 and bo.rank([-0.0, 0.0], [1, 1]) == 0   # +0 and -0 are equal
    assert bo.rank([-math.inf, -5.0], [4, 1]) == 1 and bo.rank([-math.inf, -math.inf], [4, 1]) == 0
    assert bo.rank([-1.0], [1]) == 0


def test_eot_is_counted_and_a_capped_sample_has_none():
    """Sample 0 generated [a, b, EOT] (3 log-probabilities), sample 1 stopped at the cap after [a, b] (2): each average is
    over what the sample generated.  Without EOT in the count sample 0's average would be -0.9 / 2 and lose."""
    s0 = [-0.2, -0.2, -0.5]   # the last one is EOT's
    s1 = [-0.3, -0.32]
    assert bo.rank([sum(s0), sum(s1)], [len(s0), len(s1)]) == 0           # -0.3 against -0.31
    assert bo.rank([sum(s0[:2]) + s0[2], sum(s1)], [2, 2]) == 1           # what dividing by the length without EOT gives


def test_nan_never_wins():
    nan = math.nan
    assert bo.rank([nan, -9.0, -1.0], [1, 1, 1]) == 2
    assert bo.rank([nan, -9.0], [1, 3]) == 1
    assert bo.rank([nan, nan, nan], [1, 2, 3]) == 0                        # none left: sample 0
    assert bo.rank([-1.0, -1.0], [0, 0]) == 0 and bo.rank([-1.0, -7.0], [0, 2]) == 1   # nothing counted is a NaN
    assert bo.rank([math.inf, -math.inf], [0, 1]) == 1


def test_attempt_word():
    assert bo.attempt_word(0, 0) == 0 and bo.attempt_word(3, 0) == 3      # sample 0 is the decode that draws one sample
    assert bo.attempt_word(3, 1) == 3 + 65536 and bo.attempt_word(5, 7) == 5 + 7 * 65536
    words = {bo.attempt_word(a, j) for a in range(6) for j in range(8)}   # Whisper's schedule has six attempts
    assert len(words) == 48


def toy_logits(V, salt):
    """A model of its own: logits that depend on the prefix (its length and last id) alone."""
    def fn(prefix):
        rng = np.random.default_rng([salt, len(prefix), int(prefix[-1])])
        z = rng.standard_normal(V).astype(np.float32) * 2.0
        z[7] += np.float32(0.15 * len(prefix))  # EOT = 7 grows likelier: samples end at different lengths
        return z
    return fn


def test_sample_j_is_the_decode_under_its_attempt_word():
    V, EOT, P = 300, 7, 24
    fn = toy_logits(V, 11)
    for attempt in (0, 2):
        picked, rows = bo.decode_samples(lambda w: sr.decode(fn, [1, 2], P, EOT, 3, np.float32(0.8), 5, 4, w), 5, attempt)
        plain = sr.decode(fn, [1, 2], P, EOT, 3, np.float32(0.8), 5, 4, attempt)
        assert rows[0]["ids"] == plain["ids"] and rows[0]["sum"] == plain["sum"]
        for j in range(1, 5):
            again = sr.decode(fn, [1, 2], P, EOT, 3, np.float32(0.8), 5, 4, attempt + (j << 16))
            assert rows[j]["ids"] == again["ids"] and rows[j]["lps"] == again["lps"]
        assert len({tuple(r["ids"]) for r in rows}) == 5                   # five different samples
        avgs = [r["sum"] / r["n"] for r in rows]
        assert picked == int(np.argmax(avgs)) and all(r["n"] == len(r["ids"]) - 2 for r in rows)
        assert any(r["ids"][-1] == EOT for r in rows)
    # T = 0 draws nothing: every sample is the greedy decode
    _, rows = bo.decode_samples(lambda w: sr.decode(fn, [1, 2], P, EOT, 3, np.float32(0.0), 5, 4, w), 3)
    assert rows[0]["ids"] == rows[1]["ids"] == rows[2]["ids"]


def test_pick_and_begin_reference_forms():
    rng = np.random.default_rng(2)
    N, clips, stride, c0 = 3, 4, 9, 2
    R = N * clips
    ids = rng.integers(1, 99, (R, stride))
    lp = -rng.random((R, stride)).astype(np.float32)
    n_ids = rng.integers(3, stride + 1, R).astype(np.int32)
    counts = (n_ids - 2).astype(np.int32)
    sums = np.array([lp[r, 2:n_ids[r]].astype(np.float64).sum() for r in range(R)])
    out = {"ids": np.full((8, stride), -1, np.int64), "lp": np.full((8, stride), 9.0, np.float32), "n": np.full(8, -1, np.int32),
           "count": np.full(8, -1, np.int32), "picked": np.full(8, -1, np.int32), "sum": np.full(8, 9.0),
           "all_sum": np.full((8, 8), 9.0), "all_count": np.full((8, 8), -1, np.int32)}
    o = bo.pick(ids, lp, n_ids, sums, counts, N, c0, out)
    for k in range(8):
        c = k - c0
        if not 0 <= c < clips:
            assert all(np.array_equal(o[key][k], out[key][k]) for key in out)
            continue
        j = int(np.argmax([sums[jj * clips + c] / counts[jj * clips + c] for jj in range(N)]))
        r = j * clips + c
        assert o["picked"][k] == j and o["n"][k] == n_ids[r] and o["sum"][k] == sums[r] and o["count"][k] == counts[r]
        assert list(o["ids"][k]) == list(ids[r, :n_ids[r]]) + [0] * (stride - n_ids[r])
        assert list(o["all_count"][k]) == [counts[jj * clips + c] for jj in range(N)] + [0] * 5
    prompts = np.zeros((clips, stride), np.int64)
    prompts[:, :3] = rng.integers(1, 99, (clips, 3))
    prompts[:, 3:] = 77  # (stale ids behind the prompt stay on the rows j = 0 and never reach the others)
    b_ids, b_n, b_fin, b_sum, b_count, anc = bo.begin(prompts, 3, N, stride - 1, frozen=[0, 1, 0, 0])
    assert np.array_equal(b_ids[:clips], prompts) and np.array_equal(b_ids[clips:, :3], np.tile(prompts[:, :3], (2, 1)))
    assert (b_ids[clips:, 3:] == 0).all() and (b_n == 3).all() and (b_sum == 0).all() and (b_count == 0).all()
    assert list(b_fin) == [0, 1, 0, 0] * 3
    assert list(anc[6]) == [2, 2] + [6] * (stride - 3) and list(anc[1]) == [1] * (stride - 1)


def test_debug_taps_are_exported(pkg):
    L = pkg.lib()
    for sym in ("wt_dbg_sample_select_group", "wt_dbg_best_of_begin", "wt_dbg_best_of_pick"):
        assert sym in pkg.DEBUG_SYMBOLS and hasattr(L, sym)


def test_a_null_engine_is_an_argument_error(pkg):
    """What the host ABI shows without a device: the exported symbols and the null-handle paths.  An engine cannot be
    built without one (its constructor uploads the weights), so the options' ranges and defaults and wt_last_best_of
    before any decode are asserted on the GPU (tests/test_gpu_best_of.py: test_option_range_and_refusals,
    test_fallback_beam_off_and_idle_are_the_parents_bytes)."""
    L = pkg.lib()
    invalid = [k for k, v in pkg.STATUS_NAMES.items() if v == "WT_ERR_INVALID_ARG"][0]
    assert "wt_last_best_of" in pkg.CAPI_SYMBOLS and L.wt_last_best_of(None, None, None, None, 0) == -invalid
    assert L.wt_dbg_best_of_begin(None, 1, 1, 1, 3, 2, None, None, None, None, None, None, None) == invalid
    assert L.wt_dbg_best_of_pick(None, 1, 1, 0, 1, 3, *([None] * 13)) == invalid
    assert L.wt_dbg_sample_select_group(None, 1, 1, 8, None, None, 3, 2, 2, 0, 1, 2, 50, None, 0, 0, 0, 0, -1, None, None,
                                        None, None) == invalid


# ------------------------------------------------------------ the fixtures ---
import pytest  # noqa: E402

import best_of_model as bm  # noqa: E402
import sample_model as smp  # noqa: E402
import scores_model as sm  # noqa: E402

# what best_of_model.choose_seed gave on the CPU oracle: the kept sample per clip, and the id
# counts of every sample of the first clips
PINS = {
    "ts-5x5-hot": (2, (), [3, 3, 4, 2, 4], [[22, 19, 41, 41, 41], [41, 41, 41, 41, 41], [26, 31, 33, 30, 41]]),
    "ts-2x5-cool": (3, (1,), [1, 0, 1, 1, 1], [[41, 41], [17, 17], [30, 31]]),
    "plain-2x1-long": (1, (), [0], [[23, 27]]),
    "ts-5x26-hot": (11, (), [3, 0, 4, 0, 4, 4, 3, 1, 2, 1, 1, 2, 0, 2, 3, 3, 2, 2, 4, 1, 2, 4, 0, 1, 2, 4], [[41, 41, 18, 21, 15]]),
}


@pytest.fixture(scope="module")
def ref(orc, pkg, assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    d = tmp_path_factory.mktemp("best_of")
    paths = {"ts": str(d / "micro-scores-ts"), "plain": str(d / "micro-scores-plain")}
    sm.write_ts_model(prefix + ".wtw", paths["ts"] + ".wtw")
    sm.write_plain_model(prefix + ".wtw", paths["plain"] + ".wtw")
    r = bm.make_reference(orc, paths)
    r.vocab = pkg.Vocab(vocab)
    yield r
    r.close()


@pytest.fixture(scope="module")
def gold():
    return bm.load_golden()


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and set(a) == set(b)


def test_the_pins_and_the_rule_on_clips_set_aside(gold):
    assert set(PINS) == set(bm.CASES) == set(bm.SEEDS) == set(bm.SET_ASIDE) and set(gold) == set(PINS) | {"fallback", "fallback_beam"}
    for name, (seed, aside, picked, n_ids) in PINS.items():
        mode, N, milli, clips, P = bm.CASES[name]
        g = gold[name]
        assert bm.SEEDS[name] == seed and bm.SET_ASIDE[name] == aside and 5 * len(aside) <= clips
        assert g["picked"].tolist() == picked and g["n_ids"][: len(n_ids)].tolist() == n_ids
        assert [c for c in range(clips) if not g["decisive"][c]] == list(aside)
        assert g["ids"].shape == (clips, N, P + 1) and (g["compared"] >= 1).all()
    assert {bm.CASES[n][1] for n in PINS} == {2, 5} and {bm.CASES[n][2] for n in PINS} == {200, 1000}
    # more than one sample wins somewhere, and samples of a clip end at different lengths
    assert len(set(gold["ts-5x26-hot"]["picked"].tolist())) == 5 and len(set(gold["ts-5x5-hot"]["n_ids"][0].tolist())) > 1


@pytest.mark.parametrize("name", ["ts-5x5-hot", "ts-2x5-cool", "plain-2x1-long"])
def test_the_recorded_cases_are_the_oracles(ref, gold, name):
    assert same(bm.case_arrays(ref, name), gold[name])
    ref.rows.clear()


def test_the_recorded_26_clip_case_at_its_chain_boundary(ref, gold):
    """Clips 0, 24 and 25 (the last of the first chain, the only one of the second) recomputed; all 130 samples take
    40 s on the oracle, which tests/best_of_model.py spends when it writes the file."""
    name = "ts-5x26-hot"
    mode, N, milli, clips, P = bm.CASES[name]
    g = gold[name]
    for b in (0, 24, 25):
        picked, rows = bm.clip_samples(ref, mode, b, N, milli, bm.SEEDS[name], P)
        a = bm.pack_rows([rows], P, milli)
        assert picked == g["picked"][b] and bm.decisive(rows, picked, milli) == bool(g["decisive"][b])
        assert all(np.array_equal(a[k][0], g[k][b]) for k in a), b
    ref.rows.clear()


def test_the_recorded_fallback_and_its_margins(ref, gold):
    """Every decision of every attempt lies clear of its thresholds (5e-3 on avg_logprob, 0.02 on no_speech_prob, 0.05 on
    the ratio), every sample of every attempt is decisive and an attempt's kept average is more than 2.2e-4 above that of
    any sample with other ids: the engine's fp32 scores cannot decide otherwise.  Clips are kept at T = 0 and from best-of attempts."""
    text_of = smp.text_of_vocab(ref.vocab)
    a, rows = bm.fallback_arrays(ref, text_of)
    assert same(a, gold["fallback"])
    d_avg, d_nosp, d_ratio, ok, gap = bm.fallback_margins(rows, text_of)
    print(d_avg, d_nosp, d_ratio, ok, gap)
    assert d_avg > 5e-3 and d_nosp > 0.02 and d_ratio > 0.05 and ok and gap > bm.AVG_GAP
    assert set(a["attempts"].tolist()) == {1, 2, 3}
    assert any(m == 0 for m in a["milli"]) and any(m > 0 and not n for m, n in zip(a["milli"], a["needs"]))
    assert (a["picked"][a["milli"] == 0] == 0).all() and (a["picked"] > 0).any()


def test_the_recorded_beam_fallback_and_its_margins(ref, gold):
    """Option fallback_beam: the attempt at temperature 0 is beam_full_ref.beam_search with 4 hypotheses, merged by
    sample_ref.decode_with_fallback with the best of 3 samples at 0.5 and 1.0.  Every decision lies clear of its
    thresholds as above, every search's margin is above section 23's 2e-4 and every sample decisive; clips are accepted
    from the beam and from a best-of attempt, and the beam's result differs from the greedy decode somewhere."""
    import sample_ref as sr
    assert bm.FB_K == 4 and bm.FB_N == 3 and sr.schedule(bm.FB_BEAM["temperature"], bm.FB_BEAM["temperature_increment"]) == [0, 500, 1000]
    text_of = smp.text_of_vocab(ref.vocab)
    a, rows = bm.fallback_arrays(ref, text_of, bm.FB_K)
    assert same(a, gold["fallback_beam"])
    d_avg, d_nosp, d_ratio, ok, gap = bm.fallback_margins(rows, text_of, bm.FB_BEAM)
    print(d_avg, d_nosp, d_ratio, ok, gap)
    assert d_avg > 5e-3 and d_nosp > 0.02 and d_ratio > 0.05 and ok and gap > bm.AVG_GAP
    beam_kept = [b for b, r in enumerate(rows) if r["temperature_milli"] == 0]
    assert beam_kept and all(not rows[b]["needs_fallback"] and rows[b]["margin"] > bm.BEAM_DELTA for b in beam_kept)
    assert any(r["temperature_milli"] > 0 and not r["needs_fallback"] for r in rows)  # accepted from a best-of attempt
    assert all(np.isfinite(a["margin"][b]) == (b in beam_kept) for b in range(len(rows)))
    greedy = [ref.row("ts", b, b, 0, bm.FB_BEAM["seed"], smp.P_SHORT) for b in range(len(rows))]
    assert any(r["tried"][0][1][0]["ids"] != g["ids"] for r, g in zip(rows, greedy))
    ref.rows.clear()
