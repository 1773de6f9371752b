"""Seeking long-audio transcription (options seek and condition_on_previous_text) on the GPU: the
scenario of tests/longform_model.py through transcribe_long against tests/longform_ref.py over the CPU oracle's decoder
behind the ENGINE'S OWN log-mel of every window (tests/test_longform_reference.py pins the scenario on the oracle front
end).  Without the feature set_option("seek", 1) fails and so does every test here."""
import collections
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import longform_model as lm  # noqa: E402
import longform_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
TOKEN_BOUND = 1.1e-4  # tests/test_gpu_scores.py


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def model(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("longform") / "micro-longform")
    lm.write_model(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def eng(pkg, model):
    e = pkg.Engine(model[0], model[1], True)
    e.set_option("max_positions", lm.P)
    e.set_option("timestamps", 1)
    e.set_option("scores", 1)
    e.set_option("no_speech_threshold", lm.NO_SPEECH_THRESHOLD)
    e.set_option("logprob_threshold", lm.LOGPROB_THRESHOLD)
    assert e.pcm_len == lm.WIN and e.dims.n_text_ctx == lm.N_TEXT_CTX and e.vocab_info()["prev"] == lm.PREV
    yield e
    e.close()


@pytest.fixture(scope="module")
def audio():
    x = lm.pcm()
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def reference(orc, model, eng, audio):
    """longform_ref over the oracle's decoder behind the engine's log-mel, per (condition, caller context, skip_silence),
    computed once on demand."""
    m = orc.Model(model[0] + ".wtw")
    mels, made = {}, {}

    def mel_of(seek):
        if seek not in mels:
            mels[seek] = eng.logmel_batch(lm.window(audio, seek))[0]
        return mels[seek]

    logits = lm.logits_fn_of(m, mel_of)

    def get(condition=True, context=(), skip=False):
        key = (condition, tuple(context), skip)
        if key not in made:
            dec = lr.window_decoder(logits, len(lm.PROMPT), lm.P, lm.EOT, lm.BEG, lm.NOSP,
                                    no_speech_threshold=lm.NO_SPEECH_THRESHOLD / 1000,
                                    logprob_threshold=lm.LOGPROB_THRESHOLD / 1000, skip_silence=skip)
            made[key] = lr.transcribe(dec, audio.size, lm.WIN, lm.EOT, lm.BEG, lm.PREV, lm.PROMPT, lm.KEEP, context, condition)
        return made[key]

    yield get
    m.close()


def run(eng, audio, condition=True, context=(), skip=False):
    eng.set_option("seek", 1)
    eng.set_option("condition_on_previous_text", int(condition))
    eng.set_option("skip_silence", int(skip))
    eng.set_context(list(context))
    try:
        text = eng.transcribe_long(audio)
        assert eng.get_option("context_ids") == len(context)  # the caller's context is the engine's again
        segs, seg_texts = eng.last_segments(with_text=True)
        return text, eng.last_windows(), segs, seg_texts, eng.last_scores(), eng.last_token_logprobs(lm.P + 1)
    finally:
        eng.set_option("seek", 0)
        eng.set_option("skip_silence", 0)
        eng.set_option("condition_on_previous_text", 1)
        eng.set_context([])


def check(eng, got, ws):
    text, win, segs, seg_texts, sc, lp = got
    assert lr.smallest_margin(ws) >= lm.MARGIN  # a collapsed margin fails here, loudly
    assert win.size == len(ws) == sc.size == lp.shape[0]
    for k, r in enumerate(ws):
        w = win[k]
        assert (int(w["seek_sample"]), int(w["advance_samples"]), int(w["n_context"]), int(w["n_prompt"]),
                int(w["n_kept_ids"]), int(w["skipped"]), int(w["temperature_milli"])) == \
               (r["seek"], r["advance"], r["n_context"], r["n_prompt"], len(r["kept"]), int(r.get("skipped", False)), 0), k
    lines = text.split("\n")
    assert len(lines) == len(ws)
    for line, r in zip(lines, ws):  # the window's ids, as the vocabulary prints the kept ones
        assert line == eng.decode_text(np.asarray(r["kept"], np.int64)), r["seek"]
    want = [s for r in ws for s in r["segments"]]
    assert [tuple(int(x) for x in s) for s in segs] == want
    by_window = {k: r for k, r in enumerate(ws)}
    for s, t in zip(want, seg_texts):
        assert t.decode("utf-8", errors="replace") == eng.decode_text(np.asarray(by_window[s[0]]["ids"][s[3]: s[3] + s[4]], np.int64))
    for k, r in enumerate(ws):
        n0 = r["n_prompt"]
        assert sc["n_generated"][k] == r["n"] and sc["skipped"][k] == int(r.get("skipped", False))
        assert abs(sc["no_speech_prob"][k] - r["no_speech_prob"]) <= (TOKEN_BOUND + 2.0 ** -23) * r["no_speech_prob"] + 1e-30
        err = np.abs(lp[k, n0: n0 + r["n"]].astype(np.float64) - np.asarray(r["lps"], np.float64)).max()
        assert err <= TOKEN_BOUND, (k, err)
        assert abs(sc["avg_logprob"][k] - r["avg"]) <= TOKEN_BOUND + abs(r["avg"]) * 2.0 ** -23


def test_seeking_equals_the_reference_with_condition_on_previous_text(eng, audio, reference):
    ws = reference(True)
    print([(r["seek"], r["advance"], r["branch"], r["n_context"], len(r["gen"]), len(r["kept"])) for r in ws])
    # what tests/test_longform_reference.py pins, on the engine's log-mel
    branches = collections.Counter(r["branch"] for r in ws)
    assert len(ws) >= 6 and branches["pairs"] >= 2 and branches["no_pair_stamp"] >= 2, branches
    assert sum(1 for r in ws if r["advance"] < lm.WIN and r["seek"] + lm.WIN <= lm.N_SAMPLES) >= 2
    assert any(r["n_context"] == lm.KEEP and sum(len(q["kept"]) for q in ws[:k]) > lm.KEEP for k, r in enumerate(ws))
    assert any(0 < r["n_context"] < lm.KEEP for r in ws)
    check(eng, run(eng, audio, True), ws)


def test_seeking_without_condition_on_previous_text(eng, audio, reference):
    ws, on = reference(False), reference(True)
    assert all(r["n_context"] == 0 for r in ws)
    assert any(a["gen"] != b["gen"] for a, b in zip(on, ws) if a["seek"] == b["seek"])
    check(eng, run(eng, audio, False), ws)


def test_a_caller_context_seeds_the_first_window(eng, audio, reference):
    ws = reference(True, lm.CONTEXT)
    assert ws[0]["n_context"] == len(lm.CONTEXT) and ws[0]["ids"][: 1 + len(lm.CONTEXT)] == [lm.PREV] + list(lm.CONTEXT)
    assert ws[1]["ids"][1: 1 + len(lm.CONTEXT)] == list(lm.CONTEXT)  # ... and stays in front of what the windows add
    check(eng, run(eng, audio, True, lm.CONTEXT), ws)


def test_skip_silence_blanks_windows_and_leaves_the_context_alone(eng, audio, reference):
    ws = reference(True, (), True)
    skipped = [k for k, r in enumerate(ws) if r["skipped"]]
    print("skipped windows:", skipped, ["%.3f" % r["no_speech_prob"] for r in ws])
    assert skipped and len(skipped) < len(ws)
    assert all(abs(r["no_speech_prob"] - lm.NO_SPEECH_THRESHOLD / 1000) > 0.05 for r in ws)
    for k in skipped:
        assert ws[k]["kept"] == [] and ws[k]["segments"] == [] and ws[k]["advance"] == min(lm.WIN, -(-(audio.size - ws[k]["seek"]) // 320) * 320)
    got = run(eng, audio, True, (), True)
    check(eng, got, ws)
    assert all(got[0].split("\n")[k] == "" for k in skipped)


def test_the_second_run_takes_the_single_ending_timestamp_and_the_open_segment(pkg, orc, assets, tmp_path_factory):
    """Run B of tests/longform_model.py: a window that ends in a single timestamp behind a pair (the tail is kept and the
    advance is the whole window) and one whose only timestamp is <|0.00|> (one open segment to the window's end, in file
    time), through the engine loop."""
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("longform") / "micro-longform-b")
    lm.write_model(prefix + ".wtw", p + ".wtw", lm.TS_GAIN_B)
    x = lm.pcm(amps=lm.AMPS_B, n_samples=lm.N_SAMPLES_B)
    e = pkg.Engine(p, vocab, True)
    for k, v in (("max_positions", lm.P), ("timestamps", 1), ("scores", 1), ("max_initial_timestamp", lm.MAX_INITIAL_B),
                 ("no_speech_threshold", lm.NO_SPEECH_THRESHOLD), ("logprob_threshold", lm.LOGPROB_THRESHOLD)):
        e.set_option(k, v)
    m = orc.Model(p + ".wtw")
    try:
        mel_of = lambda seek: e.logmel_batch(lm.window(x, seek))[0]  # noqa: E731
        dec = lr.window_decoder(lm.logits_fn_of(m, mel_of), len(lm.PROMPT), lm.P, lm.EOT, lm.BEG, lm.NOSP, lm.MAX_INITIAL_B,
                                lm.NO_SPEECH_THRESHOLD / 1000, lm.LOGPROB_THRESHOLD / 1000)
        ws = lr.transcribe(dec, x.size, lm.WIN, lm.EOT, lm.BEG, lm.PREV, lm.PROMPT, lm.KEEP, (), True)
        print([(r["seek"], r["advance"], r["branch"], r["n_context"], len(r["gen"]), len(r["kept"])) for r in ws])
        branches = collections.Counter(r["branch"] for r in ws)
        assert len(ws) >= 6 and branches["pairs_single_end"] >= 1 and branches["no_pair_open"] >= 1 and branches["pairs"] >= 2
        single = [r for r in ws if r["branch"] == "pairs_single_end"][0]
        assert single["advance"] == lm.WIN and single["kept"] == single["gen"]
        assert any(r["branch"] == "no_pair_open" and r["seek"] > 0 and r["segments"] and r["segments"][0][5] == 1 for r in ws)
        assert any(r["n_context"] == lm.KEEP and sum(len(q["kept"]) for q in ws[:k]) > lm.KEEP for k, r in enumerate(ws))
        check(e, run(e, x, True), ws)
    finally:
        m.close()
        e.close()


def test_seek_off_is_the_per_window_decode_as_before(eng, audio):
    n_win = -(-audio.size // lm.WIN)
    texts = [eng.transcribe(lm.window(audio, w * lm.WIN)) for w in range(n_win)]
    assert eng.get_option("seek") == 0
    assert eng.transcribe_long(audio) == "\n".join(texts)
    with pytest.raises(Exception) as e:
        eng.last_windows()  # the last synchronous decode was not a seeking one
    assert status_of(e) == INVALID


def test_seek_needs_timestamps_and_max_positions(pkg, model, audio):
    e = pkg.Engine(model[0], model[1], True)
    e.set_option("seek", 1)
    for setup in ((("max_positions", lm.P),), (("max_positions", 0), ("timestamps", 0))):
        for k, v in setup:
            e.set_option(k, v)
        with pytest.raises(pkg.WtError) as err:
            e.transcribe_long(audio[: lm.WIN])
        assert status_of(err) == UNSUPPORTED and "seek" in str(err.value)
    for bad in (-1, 2):
        for key in ("seek", "condition_on_previous_text"):
            with pytest.raises(pkg.WtError) as err:
                e.set_option(key, bad)
            assert status_of(err) == INVALID
    e.set_option("max_positions", lm.P)
    e.set_option("timestamps", 1)
    assert len(e.transcribe_long(audio[: lm.WIN + 100]).split("\n")) >= 1 and e.last_windows().size >= 1  # usable
    e.close()


def test_the_cli_flags(pkg, model, eng, audio, tmp_path):
    """encdec --long --timestamps --seek prints the segments of the in-process call on the same WAV; --no-condition and
    --context-ids reach the engine; the flags' requirements are error lines with status 105."""
    import struct
    import subprocess
    exe = os.path.join(ROOT, "whisper.tflite_amd", "bin", "encdec")
    pcm16 = np.clip(np.round(audio[: 3 * lm.WIN + 5000] * 32767), -32768, 32767).astype("<i2")
    wav = tmp_path / "long.wav"
    wav.write_bytes(b"RIFF" + struct.pack("<I", 36 + pcm16.nbytes) + b"WAVEfmt " +
                    struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" +
                    struct.pack("<I", pcm16.nbytes) + pcm16.tobytes())
    x = pkg.wav_read_legacy(str(wav))
    base = [exe, "--model-prefix", model[0], "--vocab", model[1], "--input", str(wav)]

    def stamp(ms):
        return "%02d:%02d.%03d" % (ms // 60000, ms // 1000 % 60, ms % 1000)

    def lines_of(condition, context):
        eng.set_option("scores", 0)
        try:
            got = run_plain(eng, x, condition, context)
        finally:
            eng.set_option("scores", 1)
        return ["[%s --> %s] %s" % (stamp(int(s["t0_ms"])), stamp(int(s["t1_ms"])), t.decode("utf-8", errors="replace"))
                for s, t in zip(*got)]

    def run_plain(e, pcm, condition, context):
        e.set_option("seek", 1)
        e.set_option("condition_on_previous_text", int(condition))
        e.set_context(list(context))
        try:
            e.transcribe_long(pcm)
            return e.last_segments(with_text=True)
        finally:
            e.set_option("seek", 0)
            e.set_option("condition_on_previous_text", 1)
            e.set_context([])

    for extra, condition, context in ((["--seek"], True, ()), (["--seek", "--no-condition", "--context-ids", "11,222,333"], False, (11, 222, 333))):
        r = subprocess.run(base + ["--long", "--max-positions", str(lm.P), "--timestamps"] + extra, capture_output=True,
                           text=True, errors="replace", timeout=120)
        assert r.returncode == 0, r.stderr
        want = lines_of(condition, context)
        assert want and r.stdout == "".join(line + "\n" for line in want)
    for args, line in ((["--long", "--max-positions", str(lm.P), "--seek"], "--seek requires --long --timestamps"),
                       (["--max-positions", str(lm.P), "--timestamps", "--seek"], "--seek requires --long --timestamps"),
                       (["--long", "--max-positions", str(lm.P), "--timestamps", "--no-condition"], "--no-condition requires --seek"),
                       (["--context-ids", "1,2"], "--context-ids requires --max-positions"),
                       (["--max-positions", str(lm.P), "--context-ids", "1,x"], "--context-ids: expected token ids")):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 105 and line in r.stderr, (args, r.stderr)


def test_a_window_decoded_above_temperature_half_empties_the_context(orc, model, eng, audio):
    """temperature = 0.6: every kept result was decoded above 0.5, so no window but the first is fed a context, even
    with condition_on_previous_text = 1 and a caller context; the sampler's clip index is the window index.  Windows are
    compared up to the first one whose sampled path is not decisive (sample_ref.first_indecisive)."""
    import sample_ref
    milli, seed = 600, 3
    audio = audio[: 3 * lm.WIN + 5000]  # four or five windows are enough here
    m = orc.Model(model[0] + ".wtw")
    mel_of = lambda seek: eng.logmel_batch(lm.window(audio, seek))[0]  # noqa: E731
    logits = lm.logits_fn_of(m, mel_of)

    def decode(w, seek, fed):
        r = sample_ref.decode(logits(w, seek), fed, lm.P, lm.EOT, lm.NOSP, sample_ref.temperature_of_milli(milli), seed, clip=w,
                              beg=lm.BEG, timestamps=True)
        return {"ids": r["ids"], "temperature_milli": milli, "infos": r["infos"]}

    try:
        ws = lr.transcribe(decode, audio.size, lm.WIN, lm.EOT, lm.BEG, lm.PREV, lm.PROMPT, lm.KEEP, lm.CONTEXT, True)
    finally:
        m.close()
    assert ws[0]["n_context"] == len(lm.CONTEXT) and all(r["n_context"] == 0 for r in ws[1:]) and len(ws) >= 3
    extra = 2 * 1e-4 / (milli / 1000.0)  # twice the logits bar over T, as tests/test_gpu_sampling.py
    decisive = 0
    while decisive < len(ws) and sample_ref.first_indecisive(ws[decisive]["infos"], extra) is None:
        decisive += 1
    print("windows:", len(ws), "decisive from the start:", decisive)
    assert decisive >= 2  # the reset behind window 0 and the clip index of window 1 are compared
    eng.set_option("temperature", milli)
    eng.set_option("seed", seed)
    try:
        text, win, segs, _, _, _ = run(eng, audio, True, lm.CONTEXT)
    finally:
        eng.set_option("temperature", 0)
        eng.set_option("seed", 0)
    lines = text.split("\n")
    for k in range(decisive):
        r, w = ws[k], win[k]
        assert (int(w["seek_sample"]), int(w["advance_samples"]), int(w["n_context"]), int(w["n_prompt"]), int(w["n_kept_ids"]),
                int(w["temperature_milli"])) == (r["seek"], r["advance"], r["n_context"], r["n_prompt"], len(r["kept"]), milli), k
        assert lines[k] == eng.decode_text(np.asarray(r["kept"], np.int64))
    if decisive < len(ws):  # the first indecisive window still starts where the reference's does, without a context
        assert int(win[decisive]["seek_sample"]) == ws[decisive]["seek"] and int(win[decisive]["n_context"]) == 0
