"""The definitions of tests/scores_ref.py (option scores) on hand-made tables, and the pins of
the fixtures of tests/scores_model.py on the CPU oracle, so that tests/test_gpu_scores.py cannot pass vacuously.  CPU
only."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scores_model as sm  # noqa: E402
import scores_ref as sr  # noqa: E402
import ts_ref  # noqa: E402

# a small vocabulary: text 0..5, eot 6, specials 7..9, timestamps 10..19 (as tests/test_ts_reference.py)
V, EOT, BEG = 20, 6, 10


def test_plain_logprob_is_the_log_softmax():
    rng = np.random.default_rng(0)
    z = rng.standard_normal(V).astype(np.float32) * 3
    want = z.astype(np.float64) - np.log(np.exp(z.astype(np.float64)).sum())
    for tok in (0, 7, V - 1):
        lp, den = sr.token_logprob(z, tok)
        assert lp == pytest.approx(want[tok], abs=1e-12) and den == pytest.approx(sr.logsumexp64(z))
    assert sr.no_speech_prob(z, 8) == pytest.approx(math.exp(want[8]), rel=1e-12)


def test_timestamp_logprob_is_taken_over_the_set_the_step_chose_from():
    z = np.full(V, -5.0, np.float32)
    z[2] = 1.0
    z[BEG:] = 0.0                      # rule 5 fires behind [BEG, 3]: L = log 9 > 1 (tick 0 masked by rule 3)
    g = [BEG, 3]
    tok, info = ts_ref.step(z, g, EOT, BEG)
    assert "mass" in info["fired"]
    lp, den = sr.token_logprob(z, tok, g, EOT, BEG, timestamps=True)
    assert den == pytest.approx(math.log(9.0)) and lp == pytest.approx(-math.log(9.0))
    z[2] = 2.5                         # ... and does not: text [0, eot] and ticks 1 .. 9 are all in the denominator
    tok, info = ts_ref.step(z, g, EOT, BEG)
    assert tok == 2 and "mass" not in info["fired"]
    want = math.log(math.exp(2.5) + 6 * math.exp(-5.0) + 9.0)
    lp, den = sr.token_logprob(z, tok, g, EOT, BEG, timestamps=True)
    assert den == pytest.approx(want) and lp == pytest.approx(2.5 - want)
    # the first step: timestamps 0 .. max_initial alone
    lp, den = sr.token_logprob(z, BEG + 1, [], EOT, BEG, max_initial=3, timestamps=True)
    assert den == pytest.approx(math.log(4.0))
    # text forbidden (a segment was closed): {eot} and the ticks from the last one on
    assert sr.intervals([BEG + 1, 3, BEG + 4], V, EOT, BEG) == (EOT, EOT, BEG + 4, V - 1)
    assert sr.intervals([BEG + 1], V, EOT, BEG) == (0, EOT, V, V - 1)


def test_minus_infinity_never_gives_nan():
    z = np.full(V, -np.inf, np.float32)
    assert sr.token_logprob(z, 3) == (-math.inf, -math.inf)
    assert sr.token_logprob(z, EOT, [BEG + 9, 2], EOT, BEG, timestamps=True) == (-math.inf, -math.inf)
    assert sr.no_speech_prob(z, 8) == 0.0
    z[4] = 0.0
    assert sr.token_logprob(z, 3)[0] == -math.inf and sr.token_logprob(z, 4)[0] == 0.0


def test_decode_counts_the_eot_and_nothing_behind_it():
    def fn(prefix):
        z = np.full(V, -5.0, np.float32)
        if len(prefix) == 1:
            z[8] = -5.0 + math.log(3.0)     # position 0: p(nosp) = 3 / 22
        elif len(prefix) < 5:
            z[2] = 0.0
        else:
            z[EOT] = 0.0
        return z
    r = sr.decode(fn, [7, 9], 20, EOT, 8)
    assert r["ids"] == [7, 9, 2, 2, 2, EOT] and r["n"] == 4 and len(r["lps"]) == 4
    one = -math.log(1.0 + 19 * math.exp(-5.0))
    assert r["sum"] == pytest.approx(4 * one) and r["avg"] == pytest.approx(one)
    assert r["no_speech_prob"] == pytest.approx(3.0 / 22.0)
    assert sr.decode(fn, [7, 9], 3, EOT, 8)["ids"] == [7, 9, 2, 2]   # the cap: positions 0 .. 2 fed
    assert sr.should_skip(0.7, -1.5) and not sr.should_skip(0.7, -0.5) and not sr.should_skip(0.5, -1.5)
    assert not sr.should_skip(0.6, -1.5) and sr.should_skip(0.7, -1.0)  # strict on both sides


# ------------------------------------------------------------ the fixtures ---

# what the reference gives (chosen and first computed on the CPU)
TS_N = [94, 14, 47, 77, 27, 12, 54, 88, 72, 94]
TS_N_SHORT = [38, 14, 38, 38, 27, 12, 38, 38, 38, 38]
TS_ABOVE = [3, 4, 7, 8]            # no_speech_prob above the threshold
TS_SKIP, TS_SKIP_SHORT = [3, 4], [4]  # ... of which these are skipped (7 and 8: avg_logprob above the threshold)
PLAIN_N = [20, 93, 71, 87, 16, 13, 26, 71, 39, 93, 49, 93]


def skipped(ref):
    return [b for b, r in enumerate(ref) if sr.should_skip(r["no_speech_prob"], r["avg"], sm.NO_SPEECH_THRESHOLD / 1000.0,
                                                           sm.LOGPROB_THRESHOLD / 1000.0)]


@pytest.fixture(scope="module")
def ts_rows(orc, assets, tmp_path_factory):
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("scores") / "micro-scores-ts.wtw")
    sm.write_ts_model(prefix + ".wtw", p)
    model = orc.Model(p)
    out = sm.reference(model, sm.ts_mels(), sm.P_LONG, True)
    model.close()
    return out


def test_timestamp_fixture_pins(ts_rows):
    thr = sm.NO_SPEECH_THRESHOLD / 1000.0
    nsp = [r["no_speech_prob"] for r in ts_rows]
    print("no_speech_prob:", ["%.4f" % v for v in nsp], "avg_logprob:", ["%.4f" % r["avg"] for r in ts_rows])
    assert 0.05 <= thr <= 0.95
    assert [r["n"] for r in ts_rows] == TS_N
    assert [b for b, v in enumerate(nsp) if v > thr] == TS_ABOVE
    assert len(TS_ABOVE) >= 3 and len(nsp) - len(TS_ABOVE) >= 3
    assert min(abs(v - thr) for v in nsp) > 0.02
    assert skipped(ts_rows) == TS_SKIP and set(TS_SKIP) < set(TS_ABOVE)  # a clip above the threshold is kept: high avg_logprob
    # no avg_logprob of a clip above the no-speech threshold is near the log-probability threshold
    assert min(abs(ts_rows[b]["avg"] - sm.LOGPROB_THRESHOLD / 1000.0) for b in TS_ABOVE) > 0.02
    short = sm.cut(ts_rows, sm.P_SHORT, len(sm.TS_PROMPT))
    assert [r["n"] for r in short] == TS_N_SHORT and skipped(short) == TS_SKIP_SHORT
    assert min(abs(short[b]["avg"] - sm.LOGPROB_THRESHOLD / 1000.0) for b in TS_ABOVE) > 0.02
    # the device's rule-5 decision cannot differ: the smallest |L - M| (1.48e-2) stays above the decisive margin
    gap = min(r["gap_lm"] for r in ts_rows)
    print("smallest |L - M|: %.3e, smallest top-two gap: %.3e" % (gap, min(r["gap_top"] for r in ts_rows)))
    assert gap > sm.MARGIN and min(r["gap_top"] for r in ts_rows) > sm.MARGIN
    assert 1.4e-2 < gap < 1.6e-2
    for r in ts_rows:  # the scaled id is masked by rule 1: never generated, every lp finite
        assert sm.NOSP not in r["ids"][len(sm.TS_PROMPT):] and np.isfinite(r["lps"]).all() and max(r["lps"]) <= 0.0
        assert r["sum"] == pytest.approx(sum(r["lps"])) and r["avg"] == pytest.approx(r["sum"] / r["n"])


def test_plain_fixture_pins(orc, assets, tmp_path_factory):
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("scores") / "micro-scores-plain.wtw")
    sm.write_plain_model(prefix + ".wtw", p)
    model = orc.Model(p)
    rows = sm.reference(model, sm.plain_mels(), sm.P_PLAIN, False)
    model.close()
    print("no_speech_prob:", ["%.3g" % r["no_speech_prob"] for r in rows])
    assert [r["n"] for r in rows] == PLAIN_N
    assert min(r["n"] for r in rows) < 32 - 4 and max(r["n"] for r in rows) == sm.P_PLAIN + 1 - 4
    assert any(r["ids"][-1] == sm.EOT and 40 < len(r["ids"]) < sm.P_PLAIN for r in rows)
    assert min(r["gap_top"] for r in rows) > 10 * sm.MARGIN
    assert all(1e-3 < r["no_speech_prob"] < 0.1 for r in rows)
