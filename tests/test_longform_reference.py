"""The seek rule of seeking transcription: wt_vocab_seek_step against tests/longform_ref.py on
hand-made rows of every branch and on seeded random rows that obey the timestamp rules, the Python loop on a scripted
decoder, and the pins of the scenario of tests/longform_model.py on the CPU oracle, so that tests/test_gpu_longform.py
cannot pass vacuously.  Without the feature wt_vocab_seek_step does not exist and the first tests fail.  CPU only."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import longform_model as lm  # noqa: E402
import longform_ref as lr  # noqa: E402

EOT, BEG = lm.EOT, lm.BEG
T = lambda tick: BEG + tick  # noqa: E731
WT, ST = 100, 100  # win_ticks, seg_ticks of a full micro window

# (g, win_ticks, seg_ticks, segments, advance): every branch of the rule
HAND = [
    # pairs, no single ending timestamp: cut at the second of each pair; the ids behind the last cut are dropped and the
    # advance is the tick before it
    ([T(0), 5, 6, T(20), T(20), 7, T(45), T(45), 8, 9], WT, ST, [(0, 0, 400, 0, 4, 0), (0, 400, 900, 4, 3, 0)], 45),
    # pairs and a single ending timestamp: the tail is a segment too and the whole window is consumed
    ([T(0), 5, T(20), T(20), 7, 8, T(70)], WT, ST, [(0, 0, 400, 0, 3, 0), (0, 400, 1400, 3, 4, 0)], 100),
    # no pair, with a trailing timestamp: one segment from 0 to the last timestamp
    ([T(2), 5, 6, T(61)], WT, ST, [(0, 0, 1220, 0, 4, 0)], 100),
    # no pair, without a trailing timestamp: still to the last timestamp of the row, here the opening one
    ([T(2), 5, 6, 7], WT, ST, [(0, 0, 40, 0, 4, 0)], 100),
    # no timestamp at all: to the end of the audio, open
    ([5, 6, 7], WT, ST, [(0, 0, 2000, 0, 3, 1)], 100),
    # a trailing <|0.00|> does not end the segment at 0
    ([5, 6, T(0)], WT, ST, [(0, 0, 2000, 0, 3, 1)], 100),
    ([T(0), 5, 6], WT, ST, [(0, 0, 2000, 0, 3, 1)], 100),
    # the zero-advance guard: the last cut lies behind <|0.00|>
    ([T(0), T(0), 5, 6, T(30)], WT, ST, [(0, 0, 600, 1, 4, 0)], 100),
    ([T(0), T(0), 5, 6], WT, ST, [], 100),
    ([T(0), 5, T(0), T(0), 6, 7], WT, ST, [], 100),
    # a partial last window: 37 ticks of audio
    ([T(0), 5, 6, 7], WT, 37, [(0, 0, 740, 0, 4, 1)], 37),
    ([T(0), 5, T(20), T(20), 7, 8, T(30)], WT, 37, [(0, 0, 400, 0, 3, 0), (0, 400, 600, 3, 4, 0)], 37),
    ([T(0), 5, T(20), T(20), 7], WT, 37, [(0, 0, 400, 0, 3, 0)], 20),
    # a tick past win_ticks is clamped to it, in the times and in the advance
    ([T(0), 5, T(1500), T(1500), 7], WT, ST, [(0, 0, 2000, 0, 3, 0)], 100),
    ([T(3), 5, T(140)], WT, ST, [(0, 0, 2000, 0, 3, 0)], 100),
    ([T(90), 5, T(120), T(130), 6, T(140), T(140), 7], WT, ST, [(0, 1800, 2000, 0, 3, 0)], 100),  # t0 == t1 dropped
    # a dropped empty segment: a slice with no id below EOT
    ([T(0), T(10), T(10), 5, T(20), T(20)], WT, ST, [(0, 200, 400, 2, 3, 0)], 20),
    ([T(0), 50300, T(10), T(10), 5, 6], WT, ST, [], 10),  # an id between EOT and <|0.00|> is no text
    ([T(5), 5, T(5), T(5), 6], WT, ST, [], 5),            # t0 == t1
    # n = 0 and 1
    ([], WT, ST, [], 100),
    ([], WT, 37, [], 37),
    ([T(7)], WT, ST, [], 100),
    ([5], WT, ST, [(0, 0, 2000, 0, 1, 1)], 100),
    ([T(4), T(4)], WT, ST, [], 4),
]


def test_the_python_rule_on_hand_made_rows():
    for g, wt, st, segs, adv in HAND:
        assert lr.seek_step(g, EOT, BEG, wt, st) == (segs, adv), g
    branches = collections.Counter(lr.branch(g, BEG) for g, *_ in HAND)
    assert set(branches) == {"pairs", "pairs_single_end", "no_pair_stamp", "no_pair_open"}, branches


def seg_tuples(segs):
    return [tuple(int(x) for x in s) for s in segs]


@pytest.fixture(scope="module")
def vocab(pkg, assets):
    _, path = assets("micro")
    v = pkg.Vocab(path, True)
    info = v.info()
    assert (info["eot"], info["beg"], info["prev"]) == (EOT, BEG, lm.PREV)
    yield v
    v.close()


def test_wt_vocab_seek_step_on_hand_made_rows(vocab):
    for g, wt, st, segs, adv in HAND:
        got, got_adv = vocab.seek_step(g, wt, st)
        assert (seg_tuples(got), got_adv) == (segs, adv), g


def random_row(rng, win_ticks):
    """A row the timestamp rules allow: an opening timestamp, then text, closing / opening timestamps that never
    decrease — single ones and pairs — sometimes a late tick past the window, cut anywhere (the position cap)."""
    tick = int(rng.integers(0, 5))
    g = [T(tick)]
    for _ in range(int(rng.integers(0, 6))):
        g += [int(x) for x in rng.integers(0, EOT, size=rng.integers(1, 6))]
        tick += int(rng.choice([0, 1, 7, 30, 90, 700]))
        tick = min(tick, 1500)
        g.append(T(tick))
        if rng.random() < 0.7:
            g.append(T(min(tick + int(rng.choice([0, 0, 3])), 1500)))
    if rng.random() < 0.3:
        g += [int(x) for x in rng.integers(0, EOT, size=rng.integers(1, 4))]
    return g[: int(rng.integers(0, len(g) + 1))] if rng.random() < 0.4 else g


def test_wt_vocab_seek_step_equals_the_python_on_random_rows(vocab):
    rng = np.random.default_rng(20)
    branches = collections.Counter()
    for _ in range(2500):
        wt = int(rng.choice([100, 1500]))
        st = wt if rng.random() < 0.7 else int(rng.integers(0, wt + 1))
        g = random_row(rng, wt)
        want, want_adv = lr.seek_step(g, EOT, BEG, wt, st)
        got, got_adv = vocab.seek_step(g, wt, st)
        assert (seg_tuples(got), got_adv) == (want, want_adv), (g, wt, st)
        assert 0 <= got_adv <= wt and (got_adv > 0 or st == 0)
        branches[lr.branch(g, BEG)] += 1
    print(dict(branches))
    assert min(branches[k] for k in ("pairs", "pairs_single_end", "no_pair_stamp", "no_pair_open")) >= 100, branches


def test_wt_vocab_seek_step_refuses_bad_arguments(pkg, vocab):
    for g, wt, st in (([T(0)], 0, 0), ([T(0)], 100, 101), ([T(0)], 100, -1)):
        with pytest.raises(pkg.WtError) as e:
            vocab.seek_step(g, wt, st)
        assert str(e.value).split(":")[0] == "WT_ERR_INVALID_ARG"


def test_the_fed_prompt():
    assert lr.fed_prompt([], [1, 2, 3], 9, 4) == [1, 2, 3]
    assert lr.fed_prompt([5, 6], [1, 2, 3], 9, 4) == [9, 5, 6, 1, 2, 3]
    assert lr.fed_prompt([5, 6, 7, 8, 10, 11], [1, 2, 3], 9, 4) == [9, 7, 8, 10, 11, 1, 2, 3]  # the LAST four


def test_the_python_loop_on_a_scripted_decoder():
    """Three and a bit windows of 100 ticks: the seek follows the last closed timestamp, the context collects the kept
    ids (timestamps included), a skipped window adds nothing, a hot window and condition = 0 empty the context."""
    script = {
        0: [T(0), 5, T(40), T(40), 6, 7],              # advance 40 ticks; 6, 7 are decoded again
        12800: [T(0), 6, 7, T(50)],                    # no pair: the whole window
        44800: [T(1), 8],                              # (skipped below)
        76800: [T(0), 9, T(10), T(10), 3, T(20)],
    }
    calls = []

    def decode(w, seek, fed):
        calls.append((w, seek, list(fed)))
        r = {"ids": list(fed) + script[seek] + [EOT], "skipped": seek == 44800}
        if seek == 12800:
            r["temperature_milli"] = hot
        return r

    prompt, n = [1, 2, 3], 3 * 32000 + 5000
    hot = 0
    ws = lr.transcribe(decode, n, 32000, EOT, BEG, 9, prompt, 6, context=[77], condition=True)
    assert [r["seek"] for r in ws] == [0, 12800, 44800, 76800] and [r["advance"] for r in ws] == [12800, 32000, 32000, 24320]
    assert [c[2] for c in calls] == [[9, 77, 1, 2, 3], [9, 77, T(0), 5, T(40), 1, 2, 3],
                                    [9, 5, T(40), T(0), 6, 7, T(50), 1, 2, 3], [9, 5, T(40), T(0), 6, 7, T(50), 1, 2, 3]]
    assert [r["n_context"] for r in ws] == [1, 4, 6, 6] and [r["n_prompt"] for r in ws] == [5, 8, 10, 10]
    assert ws[0]["segments"] == [(0, 0, 800, 5, 3, 0)] and ws[1]["segments"] == [(1, 800, 1800, 8, 4, 0)]
    assert ws[2]["segments"] == [] and ws[2]["kept"] == [] and ws[2]["branch"] == "skipped"
    assert ws[3]["segments"] == [(3, 4800, 5000, 10, 3, 0), (3, 5000, 5200, 13, 3, 0)] and ws[3]["branch"] == "pairs_single_end"
    del calls[:]
    hot = 600  # the second window's kept result was decoded above temperature 0.5: the context starts anew behind it
    lr.transcribe(decode, n, 32000, EOT, BEG, 9, prompt, 6, context=[77], condition=True)
    assert [c[2] for c in calls][2:] == [[1, 2, 3], [1, 2, 3]]
    del calls[:]
    hot = 0
    lr.transcribe(decode, n, 32000, EOT, BEG, 9, prompt, 6, context=[77], condition=False)
    assert [c[2] for c in calls] == [[9, 77, 1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3]]


# ------------------------------------------------------------ the fixture ---

@pytest.fixture(scope="module")
def scenario(pkg, orc, assets, vocab, tmp_path_factory):
    """Run A under both settings of condition_on_previous_text (keys True, False) and run B (key "b")."""
    prefix, _ = assets("micro")
    filters, fe, out = vocab.filters(), orc.frontend(), {}
    for name, gain, x, max_initial, conditions in (("a", lm.TS_GAIN, lm.pcm(), 50, (True, False)),
                                                   ("b", lm.TS_GAIN_B, lm.pcm(amps=lm.AMPS_B, n_samples=lm.N_SAMPLES_B),
                                                    lm.MAX_INITIAL_B, ("b",))):
        p = str(tmp_path_factory.mktemp("longform") / ("micro-longform-%s.wtw" % name))
        lm.write_model(prefix + ".wtw", p, gain)
        model = orc.Model(p)
        assert model.dims["n_text_ctx"] == lm.N_TEXT_CTX and 2 * model.dims["n_audio_ctx"] * 160 == lm.WIN
        mel_of = lambda seek: fe.logmel(lm.window(x, seek), filters, 8)  # noqa: E731
        dec = lr.window_decoder(lm.logits_fn_of(model, mel_of), len(lm.PROMPT), lm.P, EOT, BEG, lm.NOSP, max_initial,
                                lm.NO_SPEECH_THRESHOLD / 1000, lm.LOGPROB_THRESHOLD / 1000)
        for c in conditions:
            out[c] = lr.transcribe(dec, x.size, lm.WIN, EOT, BEG, lm.PREV, lm.PROMPT, lm.KEEP, (), c is not False)
        model.close()
    return out


def test_the_scenario_is_what_the_gpu_test_needs(scenario):
    """Windows, every branch of the seek rule, short advances, a truncated context, a difference between the two
    settings of condition_on_previous_text and decisive margins, over the scenario's two runs with no window set aside."""
    ws, wb = scenario[True], scenario["b"]
    for rows in (ws, wb):
        print([(r["seek"], r["advance"], r["branch"], r["n_context"], len(r["gen"]), len(r["kept"])) for r in rows])
    assert len(ws) >= 6 and len(wb) >= 6
    branches = collections.Counter(r["branch"] for r in ws)
    assert branches["pairs"] >= 2 and branches["no_pair_stamp"] >= 2, branches
    branches_b = collections.Counter(r["branch"] for r in wb)
    assert branches_b["pairs_single_end"] >= 1 and branches_b["no_pair_open"] >= 1 and branches_b["pairs"] >= 2, branches_b
    single = [r for r in wb if r["branch"] == "pairs_single_end"][0]
    assert single["advance"] == lm.WIN and single["kept"] == single["gen"]   # the tail behind the last pair is kept
    is_open = [r for r in wb if r["branch"] == "no_pair_open"][0]
    assert is_open["seek"] > 0 and is_open["segments"] == [(wb.index(is_open), is_open["seek"] // 16,
                                                            is_open["seek"] // 16 + 2000, is_open["n_prompt"], len(is_open["gen"]), 1)]
    assert all(r["gen"][0] == BEG for r in wb)  # max_initial_timestamp = 0
    assert sum(1 for r in ws if r["advance"] < lm.WIN and r["seek"] + lm.WIN <= lm.N_SAMPLES) >= 2
    assert sum(1 for r in wb if r["advance"] < lm.WIN and r["seek"] + lm.WIN <= lm.N_SAMPLES_B) >= 2
    # the context is truncated: more ids were kept before a window than it is fed
    for rows in (ws, wb):
        assert any(r["n_context"] == lm.KEEP and sum(len(q["kept"]) for q in rows[:k]) > lm.KEEP for k, r in enumerate(rows))
    assert ws[0]["n_context"] == 0 and any(0 < r["n_context"] < lm.KEEP for r in ws)
    assert ws[-1]["seek"] + lm.WIN > lm.N_SAMPLES and wb[-1]["seek"] + lm.WIN > lm.N_SAMPLES_B  # partial last windows
    off = scenario[False]
    assert all(r["n_context"] == 0 for r in off)
    assert any(a["gen"] != b["gen"] for a, b in zip(ws, off) if a["seek"] == b["seek"])
    for rows in scenario.values():
        assert lr.smallest_margin(rows) >= lm.MARGIN
    nsp = [r["no_speech_prob"] for r in ws]
    print("no-speech probabilities:", ["%.3f" % v for v in nsp])
    assert all(abs(v - lm.NO_SPEECH_THRESHOLD / 1000) > 0.05 for v in nsp)  # skip_silence decides on them alone
    assert any(v > 0.65 for v in nsp) and any(v < 0.55 for v in nsp)
