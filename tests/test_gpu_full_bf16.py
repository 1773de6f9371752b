"""Full-length decoding in the bf16 storage mode (options bf16 + full_bf16 + max_positions) on the
GPU, on the models of tests/ts_model.py (timestamps, n_text_ctx 128) and tests/full_model.py (n_text_ctx 160).

Exact checks: the first 31 ids are the bf16 31-position chain's, use_graphs 0 and 1 agree, a call repeats, switching
modes on one engine gives what fresh engines give, the refusals.

Path consistency: the oracle is fp32 and a bf16 engine may legitimately choose other ids, so the oracle is teacher-forced
along the engine's OWN ids and the engine's reported token log-probability is compared with scores_ref.token_logprob of
the same id behind the same prefix, under the mode's own rule set.  The bar is not a constant: per model, E is the
largest |logit difference| of the existing 31-position bf16 chain against the fp32 engine behind forced fp32 ids (the
machinery of test_gpu_path.py), measured when the module runs, and bar_lp = 2 * (2 * E): a log-probability is a logit
minus a log-sum-exp of logits, each within E (the inner 2), with headroom for up to 448 keys per sum instead of 31 (the
outer 2; every cached row is rounded once, so error does not accumulate along the cache).

Without the feature set_option("full_bf16", 1) fails and so does every test here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import full_model as fm  # noqa: E402
import longform_model as lm  # noqa: E402
import longform_ref as lr  # noqa: E402
import scores_ref as sr  # noqa: E402
import suppress_ref  # noqa: E402
import ts_model as tm  # noqa: E402
import ts_ref  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
PREV = 50361  # <|startofprev|> of the multilingual vocabulary
CLIPS = 4     # clips of the teacher-forced checks (the oracle runs on the CPU)
observed = {}  # (model, what) -> largest |lp - teacher-forced lp| seen


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def files(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    d = tmp_path_factory.mktemp("fullbf16")
    out = {k: (str(d / ("micro-" + k)), vocab) for k in ("ts", "rich", "dense", "long")}
    lm.write_model(prefix + ".wtw", out["long"][0] + ".wtw")
    tm.write_model(prefix + ".wtw", out["ts"][0] + ".wtw")
    fm.write_eot_rich(prefix + ".wtw", out["rich"][0] + ".wtw")
    fm.write_dense(prefix + ".wtw", out["dense"][0] + ".wtw")
    return out


@pytest.fixture(scope="module")
def mels():
    out = {"ts": tm.mels(), "rich": fm.mels(fm.RICH_CLIPS, (80, 200), fm.RICH_SEED)}
    out["long"] = out["ts"]  # (the seeking model's E is measured on the same clips; its tests decode their own audio)
    for m in out.values():
        m.setflags(write=False)
    return out


PROMPT = {"ts": tm.PROMPT, "rich": fm.RICH_PROMPT}
POSITIONS = {"ts": tm.P_LONG, "rich": 96}


def new_engine(pkg, files, model, bf16=True, positions=None, **options):
    eng = pkg.Engine(files[model][0], files[model][1], True)
    eng.set_option("max_positions", positions or POSITIONS[model])
    eng.set_option("timestamps", 0 if model == "rich" else 1)
    eng.set_option("scores", 1)
    if bf16:
        eng.set_option("bf16", 1)
        eng.set_option("full_bf16", 1)
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


@pytest.fixture(scope="module")
def bars(pkg, files, mels):
    """Per model E and bar_lp = 4 E, from the 31-position chain: bf16 logits behind forced fp32 ids against fp32 logits."""
    out = {}
    for model in ("ts", "rich", "long"):
        e = pkg.Engine(files[model][0], files[model][1], True)
        e.set_option("stop_at_eot", 0)
        mel = np.ascontiguousarray(mels[model][:CLIPS])
        ids32, _, _, lg32 = e.encdec_debug_batch(mel)
        e.set_option("bf16", 1)
        e.set_forced_ids(ids32)
        try:
            ids_f, _, _, lg16 = e.encdec_debug_batch(mel)
        finally:
            e.set_forced_ids(None)
        e.close()
        assert np.array_equal(ids_f, ids32)
        E = float(np.abs(lg16 - lg32).max())
        assert E > 1e-4  # bf16 arithmetic ran
        out[model] = {"E": E, "bar_lp": 2 * (2 * E)}
        print(f"[full_bf16] model {model}: E = {E:.4e}, bar_lp = {4 * E:.4e}")
    return out


class Oracle:
    """The CPU oracle teacher-forced along given ids: per (model, clip) the encoder output is computed once."""

    def __init__(self, orc, files, mels):
        self.orc, self.files, self.mels = orc, files, mels
        self.models, self.enc = {}, {}

    def logits_fn(self, model, clip, max_pos, mel=None):
        """clip: an index into the model's clips, or any key with the log-mel given (a window of long audio)"""
        if model not in self.models:
            self.models[model] = self.orc.Model(self.files[model][0] + ".wtw")
        m = self.models[model]
        if (model, clip) not in self.enc:
            self.enc[(model, clip)] = m.encode(self.mels[model][clip] if mel is None else mel)
        return tm.logits_fn(m, self.enc[(model, clip)], max_pos)

    def token_logprobs(self, model, clip, ids, n0, max_pos, timestamps, mit=50, mel=None, sup=None):
        """sup = (ids, first_ids): the suppression lists in front of the rules (suppress_ref.filter_row)"""
        fn = self.logits_fn(model, clip, max_pos, mel)
        if sup is not None:
            fn = suppress_ref.wrap(fn, n0, sup[0], sup[1])
        return [sr.token_logprob(fn(ids[:i]), ids[i], ids[n0:i], tm.EOT, tm.BEG, mit, timestamps)[0] for i in range(n0, len(ids))]

    def close(self):
        for m in self.models.values():
            m.close()


@pytest.fixture(scope="module")
def oracle(orc, files, mels):
    o = Oracle(orc, files, mels)
    yield o
    o.close()


def decode(eng, mel):
    ids, n = eng.encdec_tokens_full(np.ascontiguousarray(mel))
    return ids, n, eng.last_token_logprobs(ids.shape[1])


def check_path(oracle, bars, model, what, got, n0, max_pos, timestamps, mit=50, clips=None, sup=None):
    """Every generated id's reported log-probability against the oracle's behind the engine's own prefix."""
    ids, n, lp = got
    clips = list(range(ids.shape[0])) if clips is None else clips
    worst = 0.0
    for row, b in enumerate(clips):
        r = [int(x) for x in ids[row, : n[row]]]
        assert len(r) > n0 and not ids[row, n[row]:].any()
        want = np.asarray(oracle.token_logprobs(model, b, r, n0, max_pos, timestamps, mit, sup=sup), np.float64)
        have = lp[row, n0: n[row]].astype(np.float64)
        assert np.isfinite(want).all(), (what, b, "the engine chose an id the rules do not allow")
        worst = max(worst, float(np.abs(have - want).max()))
    observed[(model, what)] = worst
    print(f"[full_bf16] model {model} {what}: largest |lp - teacher-forced lp| {worst:.4e} (bar_lp {bars[model]['bar_lp']:.4e}, E {bars[model]['E']:.4e})")
    assert worst <= bars[model]["bar_lp"], (model, what, worst, bars[model])
    return worst


# ------------------------------------------------------------------------------------------------ exact checks ---
def test_the_first_31_ids_are_the_31_position_chains(pkg, files):
    """The same kernels on a larger cache (test_gpu_full_decode.py holds the same identity in fp32): exact."""
    eng = pkg.Engine(files["dense"][0], files["dense"][1], True)
    eng.set_prompt(fm.DENSE_PROMPT)
    mel = fm.dense_mels(eng.mel_shape)
    ids32_31, _ = eng.encdec_tokens_batch(mel)
    eng.set_option("bf16", 1)
    ids31, n31 = eng.encdec_tokens_batch(mel)
    assert list(n31) == [31] * 6
    eng.set_option("max_positions", fm.N_TEXT_CTX)
    with pytest.raises(pkg.WtError) as x:  # full_bf16 = 0: refused as before, and the text names both
        eng.encdec_tokens_full(mel)
    assert status_of(x) == UNSUPPORTED and "bf16" in str(x.value) and "full_bf16" in str(x.value)
    for bad in (-1, 2):
        with pytest.raises(pkg.WtError) as x:
            eng.set_option("full_bf16", bad)
        assert status_of(x) == INVALID
    assert eng.get_option("full_bf16") == 0
    eng.set_option("full_bf16", 1)
    assert eng.get_option("full_bf16") == 1
    ids, n = eng.encdec_tokens_full(mel)
    assert ids.shape == (6, fm.N_TEXT_CTX + 1) and list(n) == [fm.N_TEXT_CTX + 1] * 6
    assert np.array_equal(ids[:, :31], ids31[:, :31])
    again = eng.encdec_tokens_full(mel)  # the segment graphs replayed
    assert np.array_equal(again[0], ids) and np.array_equal(again[1], n)
    eng.set_option("use_graphs", 0)
    eager = eng.encdec_tokens_full(mel)
    assert np.array_equal(eager[0], ids) and np.array_equal(eager[1], n)
    eng.set_option("use_graphs", 1)
    eng.set_option("cross_absorb", 0)  # the cached cross-attention form, bf16 K / V
    cached = eng.encdec_tokens_full(mel)
    assert cached[0].shape == ids.shape and list(cached[1]) == list(n)
    eng.set_option("cross_absorb", 1)
    # restoring the options gives the fp32 engine's ids
    eng.set_option("max_positions", 0)
    eng.set_option("full_bf16", 0)
    eng.set_option("bf16", 0)
    back, _ = eng.encdec_tokens_batch(mel)
    assert np.array_equal(back, ids32_31)
    eng.close()


def test_switching_modes_on_one_engine_equals_fresh_engines(pkg, files, mels):
    """fp32 -> bf16 -> fp32 -> bf16 full-length calls on one engine: no call replays the other mode's graphs."""
    mel = np.ascontiguousarray(mels["ts"][:CLIPS])
    fresh = {}
    for bf in (0, 1):
        e = new_engine(pkg, files, "ts", bf16=bool(bf))
        fresh[bf] = decode(e, mel)
        e.close()
    assert not np.array_equal(fresh[0][2], fresh[1][2])  # the two modes do differ
    e = new_engine(pkg, files, "ts", bf16=False)
    e.set_option("full_bf16", 1)
    for bf in (0, 1, 0, 1):
        e.set_option("bf16", bf)
        got = decode(e, mel)
        assert np.array_equal(got[0], fresh[bf][0]) and np.array_equal(got[1], fresh[bf][1]), bf
        assert got[2].tobytes() == fresh[bf][2].tobytes(), bf
    # the beam chain's graphs likewise
    e.set_option("beam_size", 2)
    e.set_option("full_beam", 1)
    beam = {}
    for bf in (1, 0, 1, 0):
        e.set_option("bf16", bf)
        got = e.encdec_tokens_full(mel)
        if bf in beam:
            assert np.array_equal(got[0], beam[bf][0]) and np.array_equal(got[1], beam[bf][1]), bf
        beam[bf] = got
    e.close()
    for bf in (0, 1):  # every mode of the sequence against an engine that has run nothing else
        f = new_engine(pkg, files, "ts", bf16=bool(bf), beam_size=2, full_beam=1)
        want = f.encdec_tokens_full(mel)
        f.close()
        assert np.array_equal(beam[bf][0], want[0]) and np.array_equal(beam[bf][1], want[1]), bf


def test_graphs_cached_stays_bounded_behind_contexts(pkg, files, mels):
    e = new_engine(pkg, files, "ts")
    one = np.ascontiguousarray(mels["ts"][:1])
    plain = e.encdec_tokens_full(one)
    held = e.get_option("graphs_cached")
    assert held >= 1
    rng = np.random.default_rng(5)
    for n_ctx in (1, 5, 27, 60):
        e.set_context([int(i) for i in rng.integers(0, tm.EOT, size=n_ctx)])
        e.encdec_tokens_full(one)
        assert e.get_option("graphs_cached") == held, n_ctx
    e.set_context([])
    again = e.encdec_tokens_full(one)
    assert np.array_equal(again[0], plain[0]) and np.array_equal(again[1], plain[1])
    e.close()


def test_what_stays_refused_has_its_own_text(pkg, files, mels):
    e = new_engine(pkg, files, "ts")
    mel = np.ascontiguousarray(mels["ts"][:2])
    want = e.encdec_tokens_full(mel)

    def refused(fn, word="full_bf16"):
        with pytest.raises(pkg.WtError) as x:
            fn()
        assert status_of(x) == UNSUPPORTED and word in str(x.value), str(x.value)

    run = lambda: e.encdec_tokens_full(mel)
    e.set_option("word_timestamps", 1)
    refused(run)
    e.set_option("word_timestamps", 0)
    e.set_contexts([[1, 2, 3], []])
    refused(run)
    e.set_contexts([])
    language = e.get_option("language")
    e.set_option("language", -1)
    refused(run, "language")
    e.set_option("full_language", 1)
    refused(run)
    e.set_option("full_language", 0)
    e.set_option("language", language)
    e.set_option("seek", 1)
    pcm = np.zeros(e.pcm_len, np.float32)
    refused(lambda: e.transcribe_long_batch([pcm, pcm]))
    e.set_option("seek", 0)
    e.set_option("beam_size", 2)  # full_beam = 0: beam search's own refusal stands
    refused(run, "full_beam")
    e.set_option("beam_size", 1)
    e.set_option("full_bf16", 0)  # and the option off: every call is refused as before
    refused(run, "bf16")
    e.set_option("full_bf16", 1)
    got = e.encdec_tokens_full(mel)  # the engine is unharmed
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    e.close()


# -------------------------------------------------------------------------------------------- path consistency ---
def test_greedy_without_timestamps(pkg, files, mels, oracle, bars):
    eng = new_engine(pkg, files, "rich")
    mel = mels["rich"][:CLIPS]
    got = decode(eng, mel)
    check_path(oracle, bars, "rich", "greedy", got, len(fm.RICH_PROMPT), POSITIONS["rich"], False)
    assert max(int(x) for x in got[1]) > 33  # a clip runs into the long kernel's positions
    eng.set_option("cross_absorb", 0)
    check_path(oracle, bars, "rich", "greedy, cached cross-attention", decode(eng, mel), len(fm.RICH_PROMPT), POSITIONS["rich"], False)
    eng.close()
    # not a replay of the fp32 run: some log-probability differs by more than 1e-4
    f = new_engine(pkg, files, "rich", bf16=False)
    ref = decode(f, mel)
    f.close()
    same = [b for b in range(CLIPS) if np.array_equal(ref[0][b], got[0][b])]
    assert same and max(float(np.abs(ref[2][b] - got[2][b]).max()) for b in same) > 1e-4


@pytest.mark.parametrize("positions", [tm.P_LONG, tm.P_SHORT])
def test_timestamps(pkg, files, mels, oracle, bars, positions):
    eng = new_engine(pkg, files, "ts", positions=positions)
    mel = mels["ts"][:CLIPS]
    got = decode(eng, mel)
    ids, n, _ = got
    n0 = len(tm.PROMPT)
    check_path(oracle, bars, "ts", f"timestamps P {positions}", got, n0, positions, True)
    # the id-only rules of ts_ref: what a row may hold whatever the logits were
    segs = eng.last_segments()
    want = []
    for b in range(CLIPS):
        row = [int(x) for x in ids[b, : n[b]]]
        g = row[n0:]
        assert g[0] >= tm.BEG and g[0] <= tm.BEG + 50  # max_initial_timestamp
        stamps = [t for t in g if t >= tm.BEG]
        assert stamps == sorted(stamps)  # monotone
        want += ts_ref.segments(row, n0, tm.EOT, tm.BEG, clip=b)
    assert [tuple(int(x) for x in s) for s in segs] == want  # wt_last_segments parses them
    eng.set_option("max_initial_timestamp", 10)
    got10 = decode(eng, mel)
    assert all(tm.BEG <= int(got10[0][b, n0]) <= tm.BEG + 10 for b in range(CLIPS))
    if positions == tm.P_SHORT:  # (the oracle runs on the CPU: the second teacher-forced pass at the short length only)
        check_path(oracle, bars, "ts", f"timestamps P {positions} max_initial 10", got10, n0, positions, True, mit=10)
    eng.close()


def test_sampling(pkg, files, mels, oracle, bars):
    eng = new_engine(pkg, files, "ts", temperature=600, seed=7)
    mel = mels["ts"][:CLIPS]
    got = decode(eng, mel)
    check_path(oracle, bars, "ts", "sampling T 0.6", got, len(tm.PROMPT), tm.P_LONG, True)
    again = decode(eng, mel)  # same audio, options and seed: the same ids
    assert np.array_equal(again[0], got[0]) and again[2].tobytes() == got[2].tobytes()
    eng.close()


@pytest.mark.parametrize("n_ctx", [27, 200])
def test_behind_a_context(pkg, files, mels, oracle, bars, n_ctx):
    """27: the fed prompt ends at position 31 / 32; 200: truncated to the last 63 ids.  The prompt runs on the prefill kernel."""
    rng = np.random.default_rng(100 + n_ctx)
    ctx = [int(i) for i in rng.integers(0, tm.EOT, size=n_ctx)]
    keep = tm.N_TEXT_CTX // 2 - 1
    fed = [PREV] + ctx[-keep:] + list(tm.PROMPT)
    eng = new_engine(pkg, files, "ts", positions=tm.N_TEXT_CTX)
    eng.set_context(ctx)
    got = decode(eng, mels["ts"][:2])  # (two clips: behind a context the oracle is asked for every prefix anew)
    for b in range(2):
        assert [int(x) for x in got[0][b, : len(fed)]] == fed
    check_path(oracle, bars, "ts", f"context of {n_ctx} ids", got, len(fed), tm.N_TEXT_CTX, True)
    eng.close()


@pytest.mark.parametrize("K", [2, 5])
def test_beam_search(pkg, files, mels, oracle, bars, K):
    """The gathered kernel: a wrong ancestor shifts the path's log-probabilities by far more than rounding."""
    eng = new_engine(pkg, files, "ts", beam_size=K, full_beam=1)
    mel = mels["ts"][:CLIPS]
    got = decode(eng, mel)
    check_path(oracle, bars, "ts", f"beam search K {K}", got, len(tm.PROMPT), tm.P_LONG, True)
    sums, lens = eng.last_beam_scores()
    for b in range(CLIPS):
        assert lens[b] == got[1][b] - len(tm.PROMPT)
        assert abs(float(sums[b]) - float(got[2][b].astype(np.float64).sum())) < 1e-3
    again = decode(eng, mel)
    assert np.array_equal(again[0], got[0]) and again[2].tobytes() == got[2].tobytes()
    eng.set_option("use_graphs", 0)
    eager = decode(eng, mel)
    assert np.array_equal(eager[0], got[0]) and eager[2].tobytes() == got[2].tobytes()
    eng.close()


def test_best_of(pkg, files, mels, oracle, bars):
    eng = new_engine(pkg, files, "ts", temperature=600, seed=7, best_of=3)
    mel = mels["ts"][:CLIPS]
    got = decode(eng, mel)
    picked, _, _ = eng.last_best_of()
    assert picked.size == CLIPS
    check_path(oracle, bars, "ts", "best_of 3", got, len(tm.PROMPT), tm.P_LONG, True)
    eng.close()


def test_fallback_beam(pkg, files, mels, oracle, bars):
    eng = new_engine(pkg, files, "ts", beam_size=2, full_beam=1, fallback_beam=1, temperature_fallback=1, best_of=2,
                     compression_ratio_threshold=0)
    mel = mels["ts"][:CLIPS]
    got = decode(eng, mel)
    info = eng.last_decode_info()
    assert info.size == CLIPS
    check_path(oracle, bars, "ts", "fallback_beam", got, len(tm.PROMPT), tm.P_LONG, True)
    eng.close()


def test_temperature_fallback_without_beam_search(pkg, files, mels, oracle, bars):
    """The fall-back's schedule with one sample per attempt; thresholds that send some clip past temperature 0."""
    eng = new_engine(pkg, files, "ts", temperature_fallback=1, seed=7, compression_ratio_threshold=0, logprob_threshold=-300)
    mel = mels["ts"][:CLIPS]
    got = decode(eng, mel)
    info = eng.last_decode_info()
    assert info.size == CLIPS and (info["attempts"] >= 1).all()
    print("[full_bf16] temperature_fallback: attempts", [int(a) for a in info["attempts"]], "kept at", [int(t) for t in info["temperature_milli"]])
    check_path(oracle, bars, "ts", "temperature_fallback", got, len(tm.PROMPT), tm.P_LONG, True)
    again = decode(eng, mel)
    assert np.array_equal(again[0], got[0]) and again[2].tobytes() == got[2].tobytes()
    eng.close()


def test_suppress_default(pkg, files, mels, oracle, bars):
    """Whisper's default lists in front of the timestamp rules: no listed id is generated, and the reported
    log-probabilities are those of the filtered rows."""
    eng = new_engine(pkg, files, "ts", suppress_default=1)
    vocab = pkg.Vocab(files["ts"][1], True)
    a, f = vocab.default_suppress()
    vocab.close()
    a, f = [int(i) for i in a if i < tm.N_VOCAB], [int(i) for i in f if i < tm.N_VOCAB]
    assert (eng.get_option("suppress_ids"), eng.get_option("suppress_first_ids")) == (len(a), len(f)) and a
    mel = mels["ts"][:CLIPS]
    got = decode(eng, mel)
    n0 = len(tm.PROMPT)
    for b in range(CLIPS):
        assert not set(int(x) for x in got[0][b, n0: got[1][b]]) & set(a)
    check_path(oracle, bars, "ts", "suppress_default", got, n0, tm.P_LONG, True, sup=(a, f))
    eng.set_option("use_graphs", 0)
    eager = decode(eng, mel)
    assert np.array_equal(eager[0], got[0]) and eager[2].tobytes() == got[2].tobytes()
    eng.close()


def test_long_audio_in_fixed_windows(pkg, files):
    """wt_transcribe_long_pcm without seek: every window is the batch decode of that window, text, scores and
    log-probabilities; skip_silence blanks the windows the no-speech rule calls silent and nothing else."""
    eng = new_engine(pkg, files, "long", positions=lm.P)
    eng.set_option("no_speech_threshold", lm.NO_SPEECH_THRESHOLD)
    eng.set_option("logprob_threshold", lm.LOGPROB_THRESHOLD)
    audio = lm.pcm()
    n_win = -(-audio.size // lm.WIN)
    padded = np.zeros(n_win * lm.WIN, np.float32)
    padded[: audio.size] = audio
    ids, n = eng.encdec_tokens_full(eng.logmel_batch(padded.reshape(n_win, lm.WIN)))
    sc, lp = eng.last_scores(), eng.last_token_logprobs(ids.shape[1])
    text = eng.transcribe_long(audio)
    assert text == "\n".join(eng.decode_text(ids[b, : n[b]]) for b in range(n_win))
    assert eng.last_scores().tobytes() == sc.tobytes() and eng.last_token_logprobs(ids.shape[1]).tobytes() == lp.tobytes()
    silent = [b for b in range(n_win) if sr.should_skip(float(sc["no_speech_prob"][b]), float(sc["avg_logprob"][b]),
                                                        lm.NO_SPEECH_THRESHOLD / 1000, lm.LOGPROB_THRESHOLD / 1000)]
    assert silent and len(silent) < n_win  # the audio has a silent stretch
    eng.set_option("skip_silence", 1)
    lines = eng.transcribe_long(audio).split("\n")
    sk = eng.last_scores()
    assert [b for b in range(n_win) if sk["skipped"][b]] == silent
    for b in range(n_win):
        assert lines[b] == ("" if b in silent else eng.decode_text(ids[b, : n[b]]))
    eng.close()


def test_seeking_long_audio(pkg, files, oracle, bars):
    """Option seek over the scenario of tests/longform_model.py.  The loop of tests/longform_ref.py is driven with the
    bf16 engine itself as its window decoder (one call per window behind the context the loop hands over); the engine's
    own loop must give the same windows, bit for bit, and every window's log-probabilities are held against the
    oracle teacher-forced along the window's ids behind its fed prompt."""
    eng = new_engine(pkg, files, "long", positions=lm.P)
    audio = lm.pcm()
    n_tail = len(lm.PROMPT)
    mels = {}

    def decode_window(w, seek, fed):
        mels[seek] = eng.logmel_batch(lm.window(audio, seek))
        eng.set_context(fed[1: len(fed) - n_tail] if len(fed) > n_tail else [])
        ids, n, lp = decode(eng, mels[seek])
        return {"ids": [int(x) for x in ids[0, : n[0]]], "lp": lp[0].copy()}

    ws = lr.transcribe(decode_window, audio.size, lm.WIN, lm.EOT, lm.BEG, lm.PREV, lm.PROMPT, lm.KEEP)
    eng.set_context([])
    eng.set_option("seek", 1)
    text = eng.transcribe_long(audio)
    win, lp = eng.last_windows(), eng.last_token_logprobs(lm.P + 1)
    eng.set_option("seek", 0)
    assert win.size == len(ws) >= 3 and any(r["n_context"] > 0 for r in ws)
    assert any(r["advance"] < lm.WIN and r["seek"] + lm.WIN <= audio.size for r in ws)  # a window ended on a timestamp
    lines = text.split("\n")
    worst = 0.0
    for k, r in enumerate(ws):
        w = win[k]
        assert (int(w["seek_sample"]), int(w["advance_samples"]), int(w["n_context"]), int(w["n_prompt"]), int(w["n_kept_ids"])) == \
               (r["seek"], r["advance"], r["n_context"], r["n_prompt"], len(r["kept"])), k
        assert lines[k] == eng.decode_text(np.asarray(r["kept"], np.int64))
        assert lp[k].tobytes() == r["lp"].tobytes(), k
        n0, ids = r["n_prompt"], r["ids"]
        want = np.asarray(oracle.token_logprobs("long", ("seek", r["seek"]), ids, n0, lm.P, True, mel=mels[r["seek"]][0]), np.float64)
        assert np.isfinite(want).all(), k
        err = float(np.abs(lp[k, n0: len(ids)].astype(np.float64) - want).max())
        print(f"[full_bf16] seek window {k} at sample {r['seek']}: context {r['n_context']}, {len(ids) - n0} ids, largest |lp - teacher-forced lp| {err:.4e}")
        worst = max(worst, err)
    observed[("long", "seek")] = worst
    assert worst <= bars["long"]["bar_lp"], (worst, bars["long"])
    eng.close()


def test_zz_report(bars):
    for (model, what), worst in sorted(observed.items()):
        print(f"[full_bf16] {model:5s} {what:40s} {worst:.4e}  (E {bars[model]['E']:.4e}, bar_lp {bars[model]['bar_lp']:.4e})")
