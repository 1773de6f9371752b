"""Decode confidence (options scores + max_positions) on the GPU against tests/scores_ref.py over
the CPU oracle, on the models of tests/scores_model.py (tests/test_scores_reference.py pins what the reference gives on
them).  Without the feature set_option("scores", 1) fails and so does every test here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import scores_model as sm  # noqa: E402
import scores_ref as sr  # noqa: E402
import ts_ref  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
# The largest |lp - reference lp| of a token, measured on an MI355X over every call of this file (test_zz_report prints
# it), is 2.19e-5; the largest relative error of a no-speech probability is 2.25e-5.  The token's logit and the
# log-sum-exp each move by at most the logits' error against the oracle, and the project's logits bar is 1e-4
# (LOGIT_TOL), so at most 2e-4 was expected.  The bound is five times the measured per-token error.
MEASURED = 2.19e-5
TOKEN_BOUND = 5 * MEASURED
assert TOKEN_BOUND <= 5 * 2e-4
worst = {"lp": 0.0, "nsp": 0.0}


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def models(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    d = tmp_path_factory.mktemp("scores")
    ts, plain = str(d / "micro-scores-ts"), str(d / "micro-scores-plain")
    sm.write_ts_model(prefix + ".wtw", ts + ".wtw")
    sm.write_plain_model(prefix + ".wtw", plain + ".wtw")
    return {"ts": (ts, vocab), "plain": (plain, vocab)}


@pytest.fixture(scope="module")
def mels():
    out = {"ts": sm.ts_mels(), "plain": sm.plain_mels()}
    for m in out.values():
        m.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def ref(orc, models, mels):
    """scores_ref over the oracle, computed once; P_SHORT is the cut of P_LONG (test_scores_reference.py checks that)."""
    m = orc.Model(models["ts"][0] + ".wtw")
    ts = sm.reference(m, mels["ts"], sm.P_LONG, True)
    m.close()
    m = orc.Model(models["plain"][0] + ".wtw")
    plain = sm.reference(m, mels["plain"], sm.P_PLAIN, False)
    m.close()
    return {("ts", sm.P_LONG): ts, ("ts", sm.P_SHORT): sm.cut(ts, sm.P_SHORT, len(sm.TS_PROMPT)), ("plain", sm.P_PLAIN): plain}


def new_engine(pkg, models, mode, positions=None, scores=1, **kw):
    eng = pkg.Engine(models[mode][0], models[mode][1], True, **kw)
    eng.set_option("max_positions", positions or (sm.P_LONG if mode == "ts" else sm.P_PLAIN))
    eng.set_option("timestamps", 1 if mode == "ts" else 0)
    eng.set_option("scores", scores)
    return eng


@pytest.fixture(scope="module")
def engs(pkg, models):
    e = {mode: new_engine(pkg, models, mode) for mode in ("ts", "plain")}
    assert e["ts"].vocab_info()["solm"] == sm.NOSP
    yield e
    for x in e.values():
        x.close()


def decode(eng, mel):
    ids, n = eng.encdec_tokens_full(np.ascontiguousarray(mel))
    return ids, n, eng.last_scores(), eng.last_token_logprobs(ids.shape[1])


def check(got, ref_rows, n0, clips=None):
    """Ids, counts, token log-probabilities, sums, means and no-speech probabilities against the reference."""
    ids, n, sc, lp = got
    clips = list(range(len(ref_rows))) if clips is None else list(clips)
    assert ids.shape[0] == len(clips) == sc.size == lp.shape[0] and lp.shape == ids.shape
    for row, b in enumerate(clips):
        r = ref_rows[b]
        assert [int(x) for x in ids[row, : n[row]]] == r["ids"], (b, row)  # the fixtures are decisive
        want = np.asarray(r["lps"], np.float64)
        have = lp[row, n0: n[row]].astype(np.float64)
        assert not lp[row, :n0].any() and not lp[row, n[row]:].any()       # 0 for prompt ids and padding
        err = float(np.abs(have - want).max())
        worst["lp"] = max(worst["lp"], err)
        assert err <= TOKEN_BOUND, (b, err)
        assert sc["n_generated"][row] == r["n"] == n[row] - n0
        assert abs(sc["sum_logprob"][row] - r["sum"]) <= TOKEN_BOUND * r["n"] + abs(r["sum"]) * 2.0 ** -23
        assert abs(sc["avg_logprob"][row] - r["avg"]) <= TOKEN_BOUND + abs(r["avg"]) * 2.0 ** -23
        rel = abs(sc["no_speech_prob"][row] - r["no_speech_prob"]) / r["no_speech_prob"]
        worst["nsp"] = max(worst["nsp"], rel)
        assert rel <= TOKEN_BOUND + 2.0 ** -23, (b, rel)


@pytest.mark.parametrize("mode,positions", [("ts", sm.P_LONG), ("ts", sm.P_SHORT), ("plain", sm.P_PLAIN)])
def test_scores_equal_the_reference_and_ids_are_unchanged(engs, mels, ref, mode, positions):
    eng, mel = engs[mode], mels[mode]
    n0 = len(sm.TS_PROMPT if mode == "ts" else sm.PLAIN_PROMPT)
    eng.set_option("max_positions", positions)
    got = decode(eng, mel)
    check(got, ref[(mode, positions)], n0)
    assert not got[2]["skipped"].any()
    again = decode(eng, mel)  # the segment graphs replayed: the same bits
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    eng.set_option("scores", 0)
    off = eng.encdec_tokens_full(mel)  # ids and counts with the option off
    assert np.array_equal(off[0], got[0]) and np.array_equal(off[1], got[1])
    with pytest.raises(Exception) as e:
        eng.last_scores()  # the last decode ran without scores
    assert status_of(e) == INVALID
    with pytest.raises(Exception):
        eng.last_token_logprobs(positions + 1)
    eng.set_option("scores", 1)
    eng.set_option("max_positions", sm.P_LONG if mode == "ts" else sm.P_PLAIN)


@pytest.mark.parametrize("mode", ["ts", "plain"])
def test_batch_sizes_cross_attention_forms_and_eager(pkg, models, mels, ref, mode):
    """1, 5 and 64 rows; 64 clips take the absorbed cross-attention (and the cached one with cross_absorb = 0); with
    and without hipGraphs."""
    P = sm.P_LONG if mode == "ts" else sm.P_PLAIN
    n0 = len(sm.TS_PROMPT if mode == "ts" else sm.PLAIN_PROMPT)
    e = new_engine(pkg, models, mode)
    want, mel = ref[(mode, P)], mels[mode]
    pick = [b % mel.shape[0] for b in range(64)]
    mel64 = np.ascontiguousarray(mel[pick])
    assert e.get_option("cross_absorb_active") == 1
    g64 = decode(e, mel64)
    check(g64, want, n0, pick)
    check(decode(e, mel[:5]), want, n0, range(5))
    check(decode(e, mel[3:4]), want, n0, [3])
    for a, b in zip(g64, decode(e, mel64)):  # replay
        assert a.tobytes() == b.tobytes()
    e.set_option("cross_absorb", 0)
    check(decode(e, mel64), want, n0, pick)
    e.set_option("use_graphs", 0)
    check(decode(e, mel64), want, n0, pick)
    check(decode(e, mel[:5]), want, n0, range(5))
    e.set_option("cross_absorb", 1)
    for a, b in zip(g64, decode(e, mel64)):
        assert a.tobytes() == b.tobytes()
    if mode == "ts":  # the cut inside the second segment: 64 rows eager on the absorbed form, then 5 captured on the cached one
        short = ref[(mode, sm.P_SHORT)]
        e.set_option("max_positions", sm.P_SHORT)
        check(decode(e, mel64), short, n0, pick)
        e.set_option("use_graphs", 1)
        e.set_option("cross_absorb", 0)
        check(decode(e, mel[:5]), short, n0, range(5))
        check(decode(e, mel[:5]), short, n0, range(5))  # replay
    e.close()


def test_segment_scores_equal_the_python_mean(engs, mels):
    eng = engs["ts"]
    n0 = len(sm.TS_PROMPT)
    ids, n, sc, lp = decode(eng, mels["ts"])
    segs, scores = eng.last_segments(with_scores=True)
    assert segs.size == scores.size >= sm.ts_mels().shape[0]
    for s, got in zip(segs, scores):
        b, i0, cnt = int(s["clip"]), int(s["id_begin"]), int(s["id_count"])
        assert abs(got - float(lp[b, i0: i0 + cnt].astype(np.float64).mean())) <= 1e-6 * max(1.0, abs(got))
    want = []
    for b in range(ids.shape[0]):
        want += ts_ref.segments(ids[b, : n[b]], n0, sm.EOT, sm.BEG, clip=b)
    assert [tuple(int(x) for x in s) for s in segs] == want


def test_long_audio_scores_per_window(engs):
    eng = engs["ts"]
    n0 = len(sm.TS_PROMPT)
    rng = np.random.default_rng(42)
    pcm = (0.1 * rng.standard_normal((2, eng.pcm_len))).astype(np.float32)
    ids, n = eng.encdec_tokens_full(eng.logmel_batch(pcm))
    sc, lp = eng.last_scores(), eng.last_token_logprobs(ids.shape[1])
    text = eng.transcribe_long(pcm.reshape(-1))
    assert text == "\n".join(eng.decode_text(ids[b, : n[b]]) for b in range(2))
    sc2, lp2 = eng.last_scores(), eng.last_token_logprobs(ids.shape[1])
    assert sc2.size == 2 and sc2.tobytes() == sc.tobytes() and lp2.tobytes() == lp.tobytes()  # one per window
    segs, scores = eng.last_segments(with_scores=True)
    assert segs.size == scores.size and any(int(s["clip"]) == 1 for s in segs)
    for s, got in zip(segs, scores):
        b, i0, cnt = int(s["clip"]), int(s["id_begin"]), int(s["id_count"])
        assert abs(got - float(lp[b, i0: i0 + cnt].astype(np.float64).mean())) <= 1e-6 * max(1.0, abs(got))
    one = eng.transcribe(pcm[1])
    assert one == eng.decode_text(ids[1, : n[1]]) and eng.last_scores().tobytes() == sc[1:].tobytes()
    assert n0 == 3


def test_option_off_changes_nothing(pkg, models, mels):
    three = np.ascontiguousarray(mels["plain"][:3])
    plain = pkg.Engine(models["plain"][0], models["plain"][1], True)  # never had the option
    plain.set_option("max_positions", sm.P_PLAIN)
    want_full = plain.encdec_tokens_full(three)
    plain.set_option("max_positions", 0)
    want31 = plain.encdec_tokens_batch(three)
    with pytest.raises(pkg.WtError) as e:
        plain.last_scores()
    assert status_of(e) == INVALID
    plain.close()
    eng = new_engine(pkg, models, "plain")
    assert eng.get_option("scores") == 1 and eng.get_option("skip_silence") == 0
    assert eng.get_option("no_speech_threshold") == 600 and eng.get_option("logprob_threshold") == -1000
    with_sc = eng.encdec_tokens_full(three)
    assert np.array_equal(with_sc[0], want_full[0]) and np.array_equal(with_sc[1], want_full[1])
    assert eng.last_scores().size == 3
    eng.set_option("scores", 0)
    off = eng.encdec_tokens_full(three)  # off again: the ids of an engine that never had it
    assert np.array_equal(off[0], want_full[0]) and np.array_equal(off[1], want_full[1])
    with pytest.raises(pkg.WtError) as e:
        eng.last_scores()
    assert status_of(e) == INVALID
    eng.set_option("scores", 1)
    eng.encdec_tokens_full(three)
    eng.set_option("scores", 0)
    eng.set_option("max_positions", 0)
    got31 = eng.encdec_tokens_batch(three)  # after a scores call an ordinary 31-position call gives its old ids
    assert np.array_equal(got31[0], want31[0]) and np.array_equal(got31[1], want31[1])
    for getter in (eng.last_scores, lambda: eng.last_token_logprobs(32)):  # ... and leaves no scores behind
        with pytest.raises(pkg.WtError) as e:
            getter()
        assert status_of(e) == INVALID
    eng.close()


def test_defaults_after_a_skipped_scores_decode(pkg, models):
    """Scores of an earlier call never reach a later one: after a decode whose every clip was skipped, the 31-position
    text entry points (every option back at its default) return their old text, for more windows than that decode had
    clips too, and the getters report that no scores exist."""
    rng = np.random.default_rng(5)
    eng = pkg.Engine(models["ts"][0], models["ts"][1], True)
    pcm = (0.1 * rng.standard_normal((3, eng.pcm_len))).astype(np.float32)
    old = [eng.transcribe(pcm[b]) for b in range(3)]
    old_long = eng.transcribe_long(pcm.reshape(-1))
    assert all(old) and old_long == "\n".join(old)
    eng.set_option("max_positions", 64)
    eng.set_option("timestamps", 1)
    eng.set_option("scores", 1)
    eng.set_option("skip_silence", 1)
    eng.set_option("no_speech_threshold", 0)   # every no-speech probability is above 0 ...
    eng.set_option("logprob_threshold", 0)     # ... and no avg_logprob is: every clip is skipped
    assert eng.transcribe(pcm[0]) == "" and eng.last_scores()["skipped"][0] == 1  # ONE clip, skipped
    for k, v in (("skip_silence", 0), ("scores", 0), ("timestamps", 0), ("max_positions", 0)):
        eng.set_option(k, v)
    assert eng.transcribe_long(pcm.reshape(-1)) == old_long   # three windows behind a one-clip scores decode
    assert [eng.transcribe(pcm[b]) for b in range(3)] == old
    with pytest.raises(pkg.WtError) as e:
        eng.last_scores()
    assert status_of(e) == INVALID
    # a full-length call without scores behind a skipped one keeps its text as well
    eng.set_option("max_positions", 64)
    full = eng.transcribe(pcm[0])
    eng.set_option("scores", 1)
    eng.set_option("skip_silence", 1)
    assert eng.transcribe(pcm[0]) == ""
    eng.set_option("skip_silence", 0)
    eng.set_option("scores", 0)
    assert eng.transcribe(pcm[0]) == full and full
    eng.close()


@pytest.mark.parametrize("positions", [sm.P_LONG, sm.P_SHORT])
def test_skip_silence_on_the_fixture(pkg, models, mels, ref, positions):
    """Both halves of Whisper's rule with the pinned thresholds: the reference's clips are flagged and lose their
    segments, the id rows stay."""
    rows = ref[("ts", positions)]
    want = [b for b, r in enumerate(rows) if sr.should_skip(r["no_speech_prob"], r["avg"], sm.NO_SPEECH_THRESHOLD / 1000.0,
                                                            sm.LOGPROB_THRESHOLD / 1000.0)]
    above = [b for b, r in enumerate(rows) if r["no_speech_prob"] > sm.NO_SPEECH_THRESHOLD / 1000.0]
    assert want and set(want) < set(above)
    eng = new_engine(pkg, models, "ts", positions)
    plain_ids = eng.encdec_tokens_full(mels["ts"])
    all_segs = eng.last_segments()
    eng.set_option("skip_silence", 1)
    eng.set_option("logprob_threshold", sm.LOGPROB_THRESHOLD)
    got = decode(eng, mels["ts"])
    assert np.array_equal(got[0], plain_ids[0]) and np.array_equal(got[1], plain_ids[1])  # the id rows are left alone
    assert [b for b in range(len(rows)) if got[2]["skipped"][b]] == want
    segs = eng.last_segments()
    keep = [tuple(int(x) for x in s) for s in all_segs if int(s["clip"]) not in want]
    assert [tuple(int(x) for x in s) for s in segs] == keep and len(keep) < all_segs.size
    assert eng.last_segments(with_scores=True)[1].size == len(keep)
    eng.close()


def test_skip_silence_in_the_text_entry_points(pkg, orc, models):
    """Windows of noise at several levels through the text entry points: the no-speech threshold is put into the widest
    gap of the REFERENCE's probabilities (the oracle on the engine's log-mel); logprob_threshold = 0 lets it decide alone."""
    eng = new_engine(pkg, models, "ts", 64)
    rng = np.random.default_rng(11)
    amps = (0.01, 0.03, 0.08, 0.2, 0.5, 1.0)
    pcm = np.stack([(a * rng.standard_normal(eng.pcm_len)).astype(np.float32) for a in amps])
    mel = eng.logmel_batch(pcm)
    m = orc.Model(models["ts"][0] + ".wtw")
    rows = sm.reference(m, mel, 64, True)
    m.close()
    nsp = sorted(r["no_speech_prob"] for r in rows)
    gaps = [(nsp[i + 1] - nsp[i], i) for i in range(len(nsp) - 1)]
    gap, i = max(gaps)
    assert gap > 0.04, nsp
    thr = int(round(500.0 * (nsp[i] + nsp[i + 1])))
    want = [r["no_speech_prob"] > thr / 1000.0 for r in rows]
    assert any(want) and not all(want)
    texts = [eng.transcribe(pcm[b]) for b in range(len(amps))]
    assert all(texts)
    eng.set_option("skip_silence", 1)
    eng.set_option("no_speech_threshold", thr)
    eng.set_option("logprob_threshold", 0)
    for b in range(len(amps)):
        assert eng.transcribe(pcm[b]) == ("" if want[b] else texts[b])
        assert bool(eng.last_scores()["skipped"][0]) == want[b]
        if want[b]:
            assert eng.last_segments().size == 0
    long_text = eng.transcribe_long(pcm.reshape(-1))
    lines = long_text.split("\n")
    assert len(lines) == len(amps)  # the line count is preserved
    assert lines == ["" if want[b] else texts[b] for b in range(len(amps))]
    assert [bool(x) for x in eng.last_scores()["skipped"]] == want
    assert not any(want[int(s["clip"])] for s in eng.last_segments())
    eng.close()


def test_refusals(pkg, models, mels, assets):
    from conftest import DevBuf
    three = np.ascontiguousarray(mels["plain"][:3])
    eng = pkg.Engine(models["plain"][0], models["plain"][1], True)
    parent_ids, parent_n = eng.encdec_tokens_batch(three)
    keys = ("scores", "skip_silence", "max_positions", "beam_size", "bf16", "language")

    def refused(fn, code=UNSUPPORTED):
        with pytest.raises(pkg.WtError) as e:
            fn()
        assert status_of(e) == code, str(e.value)
        assert len(str(e.value).split(":", 1)[1].strip()) > 0  # a wt_last_error text
        keep = {k: eng.get_option(k) for k in keys}  # the engine stays usable: a default call gives the parent's ids
        for k, v in (("skip_silence", 0), ("scores", 0), ("max_positions", 0), ("beam_size", 1), ("bf16", 0), ("language", 2)):
            eng.set_option(k, v)
        ids, n = eng.encdec_tokens_batch(three)
        assert np.array_equal(ids, parent_ids) and np.array_equal(n, parent_n)
        for k in ("language", "bf16", "beam_size", "max_positions", "scores", "skip_silence"):
            eng.set_option(k, keep[k])

    for key in ("scores", "skip_silence"):
        for bad in (-1, 2):
            with pytest.raises(pkg.WtError) as e:
                eng.set_option(key, bad)
            assert status_of(e) == INVALID
    eng.set_option("scores", 1)
    dev = DevBuf(three)
    pcm = np.zeros(1600, np.float32)
    # without max_positions: every decode call
    refused(lambda: eng.encdec_tokens_batch(three))
    refused(lambda: eng.encdec_tokens_batch_dev(dev.data_ptr(), 3))
    refused(lambda: eng.encdec_tokens_full(three, ids_stride=sm.P_PLAIN + 1))
    refused(lambda: eng.transcribe(pcm))
    refused(lambda: eng.transcribe_long(pcm))
    refused(lambda: eng.pipeline_submit_dev(dev.data_ptr(), 3))
    eng._submitted = []
    assert eng.get_option("in_flight") == 0
    # with it: whatever max_positions refuses
    eng.set_option("max_positions", sm.P_PLAIN)
    refused(lambda: eng.encdec_tokens_batch(three))                # the [B][32] calls
    refused(lambda: eng.pipeline_submit_dev(dev.data_ptr(), 3))    # the pipeline
    eng._submitted = []
    eng.set_option("beam_size", 4)
    refused(lambda: eng.encdec_tokens_full(three))
    eng.set_option("beam_size", 1)
    eng.set_option("bf16", 1)
    refused(lambda: eng.encdec_tokens_full(three))
    eng.set_option("bf16", 0)
    eng.set_option("language", pkg.WT_LANGUAGE_AUTO)
    refused(lambda: eng.encdec_tokens_full(three))
    eng.set_option("language", 2)
    # skip_silence without scores
    eng.set_option("scores", 0)
    eng.set_option("skip_silence", 1)
    refused(lambda: eng.encdec_tokens_full(three))
    refused(lambda: eng.transcribe(pcm))
    eng.set_option("skip_silence", 0)
    eng.set_option("scores", 1)
    dev.free()
    eng.encdec_tokens_full(three)  # everything restored: a scores call works
    assert eng.last_scores().size == 3
    eng.close()
    # a vocabulary without the no-speech id: the option itself is refused
    prefix, vocab = assets("micro")
    small = pkg.Engine(prefix, vocab, True)
    with pytest.raises(pkg.WtError) as e:
        small.set_option("scores", 1)
    assert status_of(e) == UNSUPPORTED and small.get_option("scores") == 0
    small.close()


def test_zz_report():
    print("largest |lp - reference lp| per token: %.3e; largest relative no_speech_prob error: %.3e" % (worst["lp"], worst["nsp"]))
