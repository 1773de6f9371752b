"""Batched seeking transcription (wt_transcribe_long_batch) on the GPU: the four files of
tests/longform_batch_model.py side by side, against tests/longform_ref.py PER FILE over the CPU oracle's decoder behind
the ENGINE'S OWN log-mel of every window — the method of tests/test_gpu_longform.py; tests/test_longform_batch_reference.py
pins the scenario on the oracle front end.  Without the feature Engine.transcribe_long_batch does not exist and every test
here fails."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import longform_batch_model as bm  # noqa: E402
import longform_model as lm  # noqa: E402
import longform_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
TOKEN_BOUND = 1.1e-4  # tests/test_gpu_scores.py
N_FILES = len(bm.FILES)


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def model(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("longform_batch") / "micro-longform")
    lm.write_model(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def eng(pkg, model):
    e = pkg.Engine(model[0], model[1], True)
    for k, v in (("max_positions", bm.P), ("timestamps", 1), ("scores", 1), ("no_speech_threshold", lm.NO_SPEECH_THRESHOLD),
                 ("logprob_threshold", lm.LOGPROB_THRESHOLD)):
        e.set_option(k, v)
    assert e.pcm_len == bm.WIN and e.dims.n_text_ctx == lm.N_TEXT_CTX and e.vocab_info()["prev"] == lm.PREV
    yield e
    e.close()


@pytest.fixture(scope="module")
def audio():
    xs = [bm.pcm(f) for f in range(N_FILES)]
    for x in xs:
        x.setflags(write=False)
    return xs


@pytest.fixture(scope="module")
def reference(orc, model, eng, audio):
    """Per (variant, file): longform_ref over the oracle's decoder behind the engine's log-mel, computed once on demand;
    the encoder outputs are shared by the variants."""
    m = orc.Model(model[0] + ".wtw")
    mels, made = {}, {}

    def mel_of(f, x, seek):
        if (f, x.size, seek) not in mels:  # (a file cut short pads its last window earlier)
            mels[(f, x.size, seek)] = eng.logmel_batch(lm.window(x, seek))[0]
        return mels[(f, x.size, seek)]

    def get(variant, f, n=None):  # n: the file cut to its first n samples
        x = audio[f] if n is None else audio[f][:n]
        if (variant, f, x.size) not in made:
            made[(variant, f, x.size)] = bm.reference(m, mel_of, f, variant, x)
        return made[(variant, f, x.size)]

    yield get
    m.close()


def options(eng, variant):
    condition, context, skip = variant
    eng.set_option("condition_on_previous_text", int(condition))
    eng.set_option("skip_silence", int(skip))
    eng.set_context(list(context))


def restore(eng):
    eng.set_option("seek", 0)
    eng.set_option("skip_silence", 0)
    eng.set_option("condition_on_previous_text", 1)
    eng.set_context([])


def results(eng, texts):
    segs, seg_texts, seg_sc = eng.last_segments(with_text=True, with_scores=True)
    return {"texts": texts, "win": eng.last_windows(), "files": eng.last_window_files(), "segs": segs, "seg_texts": seg_texts,
            "sc": eng.last_scores(), "lp": eng.last_token_logprobs(bm.P + 1), "seg_sc": seg_sc}


def run_batch(eng, xs, variant):
    options(eng, variant)
    try:
        texts = eng.transcribe_long_batch(xs)
        assert eng.get_option("context_ids") == len(variant[1]) and eng.get_option("context_clips") == 0  # the caller's again
        return results(eng, texts)
    finally:
        restore(eng)


def run_alone(eng, x, variant):
    options(eng, variant)
    eng.set_option("seek", 1)
    try:
        text = eng.transcribe_long(x)
        segs, seg_texts, seg_sc = eng.last_segments(with_text=True, with_scores=True)
        return {"texts": [text], "win": eng.last_windows(), "segs": segs, "seg_texts": seg_texts, "sc": eng.last_scores(),
                "lp": eng.last_token_logprobs(bm.P + 1), "seg_sc": seg_sc}
    finally:
        restore(eng)


def check(eng, got, runs):
    """got: a batch call's results over the files whose reference runs are `runs`, file by file."""
    win, files, sc, lp = got["win"], got["files"], got["sc"], got["lp"]
    assert [lr.smallest_margin(ws) >= bm.MARGIN for ws in runs] == [True] * len(runs)  # a collapsed margin fails here, loudly
    flat = [(f, k, r) for f, ws in enumerate(runs) for k, r in enumerate(ws)]
    assert win.size == len(flat) == sc.size == lp.shape[0] == files.size
    assert [int(f) for f in files] == [f for f, _, _ in flat]
    for i, (f, k, r) in enumerate(flat):
        w = win[i]
        assert (int(w["seek_sample"]), int(w["advance_samples"]), int(w["n_context"]), int(w["n_prompt"]),
                int(w["n_kept_ids"]), int(w["skipped"]), int(w["temperature_milli"])) == \
               (r["seek"], r["advance"], r["n_context"], r["n_prompt"], len(r["kept"]), int(r.get("skipped", False)), 0), (f, k)
        n0 = r["n_prompt"]
        assert sc["n_generated"][i] == r["n"] and sc["skipped"][i] == int(r.get("skipped", False))
        assert abs(sc["no_speech_prob"][i] - r["no_speech_prob"]) <= (TOKEN_BOUND + 2.0 ** -23) * r["no_speech_prob"] + 1e-30
        err = np.abs(lp[i, n0: n0 + r["n"]].astype(np.float64) - np.asarray(r["lps"], np.float64)).max()
        assert err <= TOKEN_BOUND, (f, k, err)
        assert abs(sc["avg_logprob"][i] - r["avg"]) <= TOKEN_BOUND + abs(r["avg"]) * 2.0 ** -23
    base = np.cumsum([0] + [len(ws) for ws in runs])
    for f, ws in enumerate(runs):
        lines = got["texts"][f].split("\n")
        assert len(lines) == len(ws)
        for line, r in zip(lines, ws):  # the window's ids, as the vocabulary prints the kept ones
            assert line == eng.decode_text(np.asarray(r["kept"], np.int64)), (f, r["seek"])
    # segments: clip = the window's index in the whole list, times in the file
    want = [(int(base[f]) + s[0],) + tuple(s[1:]) for f, ws in enumerate(runs) for r in ws for s in r["segments"]]
    assert [tuple(int(x) for x in s) for s in got["segs"]] == want
    for s, t in zip(want, got["seg_texts"]):
        r = flat[s[0]][2]
        assert t.decode("utf-8", errors="replace") == eng.decode_text(np.asarray(r["ids"][s[3]: s[3] + s[4]], np.int64))
    assert got["seg_sc"].size == len(want)
    for s, v in zip(want, got["seg_sc"]):  # the mean over the segment's ids below EOT
        r = flat[s[0]][2]
        lps = [r["lps"][i - r["n_prompt"]] for i in range(s[3], s[3] + s[4]) if r["ids"][i] < lm.EOT]
        assert abs(v - np.mean(lps)) <= TOKEN_BOUND + abs(np.mean(lps)) * 2.0 ** -23


@pytest.mark.parametrize("variant", bm.VARIANTS, ids=["scenario", "no_condition", "caller_context_no_skip"])
def test_every_file_equals_its_reference(eng, audio, reference, variant):
    # the scenario whole; the other settings on the heads of files 0 and 1 next to file 2, which keeps their references short
    cuts = [None] * N_FILES if variant == bm.SCENARIO else [3 * bm.WIN + 5000, 3 * bm.WIN, None]
    xs = [audio[f] if n is None else audio[f][:n] for f, n in enumerate(cuts)]
    runs = [reference(variant, f, n) for f, n in enumerate(cuts)]
    for f, ws in enumerate(runs):
        print(f, [(r["seek"], r["advance"], r["n_context"], r["n_prompt"], len(r["ids"]), int(r["skipped"]), len(r["kept"])) for r in ws])
    if variant == bm.SCENARIO:  # what tests/test_longform_batch_reference.py pins, on the engine's log-mel
        lengths = [sorted({r["n_prompt"] for _, r in rd}) for rd in bm.rounds(runs)]
        assert sum(1 for s in lengths if len(s) >= 3) >= 3, lengths
        assert any({0, bm.KEEP} <= {r["n_context"] for _, r in rd} for rd in bm.rounds(runs))
    if variant[1]:
        assert all(ws[0]["n_context"] == len(variant[1]) for ws in runs)  # the caller's context seeds every file
    if not variant[0]:
        assert all(r["n_context"] == 0 for ws in runs for r in ws)
    check(eng, run_batch(eng, xs, variant), runs)


def test_the_batch_equals_every_file_alone_and_leaves_the_single_file_call_unchanged(eng, audio):
    """Per file bit for bit in ids, windows and segments (the scores within the token bar: a batch of one takes the
    cached cross-attention, as the files alone do); one file through the batch call; transcribe_long before and after."""
    variant = bm.SCENARIO
    before = run_alone(eng, audio[1], variant)
    got = run_batch(eng, audio, variant)
    base = np.cumsum([0] + [int((got["files"] == f).sum()) for f in range(N_FILES)])
    for f in range(N_FILES):
        alone = before if f == 1 else run_alone(eng, audio[f], variant)
        sl = slice(int(base[f]), int(base[f + 1]))
        assert got["texts"][f] == alone["texts"][0]
        assert got["win"][sl].tobytes() == alone["win"].tobytes()
        mine = got["segs"][(got["segs"]["clip"] >= base[f]) & (got["segs"]["clip"] < base[f + 1])].copy()
        mine["clip"] -= base[f]
        assert mine.tobytes() == alone["segs"].tobytes()
        assert np.array_equal(got["sc"]["n_generated"][sl], alone["sc"]["n_generated"])
        assert np.abs(got["lp"][sl] - alone["lp"]).max() <= TOKEN_BOUND
        one = run_batch(eng, [audio[f]], variant)  # n_files = 1
        assert one["texts"] == alone["texts"] and one["win"].tobytes() == alone["win"].tobytes()
        assert one["segs"].tobytes() == alone["segs"].tobytes() and not one["files"].any()
    after = run_alone(eng, audio[1], variant)
    for k in ("texts", "seg_texts"):
        assert after[k] == before[k]
    for k in ("win", "segs", "sc", "lp", "seg_sc"):
        assert after[k].tobytes() == before[k].tobytes(), k
    with pytest.raises(Exception) as e:
        eng.last_window_files()  # the last synchronous decode was not a batch call
    assert status_of(e) == INVALID


def test_a_run_at_temperature_against_sample_ref(orc, model, eng, audio):
    """temperature = 0.6: window w of a file has clip index w in the sampler's counter and its own positions, whatever
    the file's place in the batch; every kept result empties the context.  Files are compared up to their first window
    whose sampled path is not decisive (sample_ref.first_indecisive)."""
    import sample_ref
    milli, seed = 600, 3
    xs = [audio[0][: 2 * bm.WIN + 5000], audio[1][: 2 * bm.WIN], audio[2]]
    m = orc.Model(model[0] + ".wtw")
    runs = []
    try:
        for f, x in enumerate(xs):
            logits = lm.logits_fn_of(m, lambda seek, x=x: eng.logmel_batch(lm.window(x, seek))[0])

            def decode(w, seek, fed, logits=logits):
                r = sample_ref.decode(logits(w, seek), fed, bm.P, lm.EOT, lm.NOSP, sample_ref.temperature_of_milli(milli), seed, clip=w,
                                      beg=lm.BEG, timestamps=True)
                return {"ids": r["ids"], "temperature_milli": milli, "infos": r["infos"]}

            runs.append(lr.transcribe(decode, x.size, bm.WIN, lm.EOT, lm.BEG, lm.PREV, lm.PROMPT, bm.KEEP, lm.CONTEXT, True))
    finally:
        m.close()
    extra = 2 * 1e-4 / (milli / 1000.0)  # twice the logits bar over T, as tests/test_gpu_sampling.py
    eng.set_option("temperature", milli)
    eng.set_option("seed", seed)
    try:
        got = run_batch(eng, xs, (True, lm.CONTEXT, False))
    finally:
        eng.set_option("temperature", 0)
        eng.set_option("seed", 0)
    compared = 0
    for f, ws in enumerate(runs):
        win = got["win"][got["files"] == f]
        lines = got["texts"][f].split("\n")
        decisive = 0
        while decisive < len(ws) and sample_ref.first_indecisive(ws[decisive]["infos"], extra) is None:
            decisive += 1
        for k in range(min(decisive, len(win))):
            r, w = ws[k], win[k]
            assert (int(w["seek_sample"]), int(w["advance_samples"]), int(w["n_context"]), int(w["n_prompt"]), int(w["n_kept_ids"]),
                    int(w["temperature_milli"])) == (r["seek"], r["advance"], r["n_context"], r["n_prompt"], len(r["kept"]), milli), (f, k)
            assert lines[k] == eng.decode_text(np.asarray(r["kept"], np.int64))
        compared += decisive
        print("file", f, "windows", len(ws), "decisive from the start", decisive)
    assert compared >= 3  # the per-file clip index of a second window is among them


def test_refusals(pkg, model, eng, audio):
    def refused(fn, status, word=None):
        with pytest.raises(pkg.WtError) as err:
            fn()
        assert status_of(err) == status, str(err.value)
        if word:
            assert word in str(err.value)

    short = [audio[2], audio[2]]
    refused(lambda: eng.transcribe_long_batch([]), INVALID)
    refused(lambda: eng.transcribe_long_batch([audio[2]] * 65), UNSUPPORTED, "64")
    eng.set_option("word_timestamps", 1)
    try:
        refused(lambda: eng.transcribe_long_batch(short), UNSUPPORTED, "word_timestamps")
    finally:
        eng.set_option("word_timestamps", 0)
    for key, bad, good in (("beam_size", 2, 1), ("bf16", 1, 0), ("language", -1, eng.get_option("language"))):
        eng.set_option(key, bad)
        try:
            refused(lambda: eng.transcribe_long_batch(short), UNSUPPORTED)
        finally:
            eng.set_option(key, good)
    e = pkg.Engine(model[0], model[1], True)
    refused(lambda: e.transcribe_long_batch(short), UNSUPPORTED)  # neither timestamps nor max_positions
    e.close()
    assert len(eng.transcribe_long_batch(short)) == 2  # ... and the engine is usable


def test_the_cli_prints_every_file_under_its_path(pkg, model, eng, audio, tmp_path):
    exe = os.path.join(ROOT, "whisper.tflite_amd", "bin", "encdec")
    paths, xs = [], []
    for f in (1, 2):
        pcm16 = np.clip(np.round(audio[f][: 2 * bm.WIN + 5000] * 32767), -32768, 32767).astype("<i2")
        wav = tmp_path / ("f%d.wav" % f)
        wav.write_bytes(b"RIFF" + struct.pack("<I", 36 + pcm16.nbytes) + b"WAVEfmt " +
                        struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" +
                        struct.pack("<I", pcm16.nbytes) + pcm16.tobytes())
        paths.append(str(wav))
        xs.append(pkg.wav_read_legacy(str(wav)))
    eng.set_option("scores", 0)
    try:
        texts = run_plain(eng, xs)
    finally:
        eng.set_option("scores", 1)
    base = [exe, "--model-prefix", model[0], "--vocab", model[1]]
    r = subprocess.run(base + ["--inputs", ",".join(paths), "--long", "--max-positions", str(bm.P), "--timestamps", "--seek"],
                       capture_output=True, text=True, errors="replace", timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "".join("== %s\n%s\n" % (p, t) for p, t in zip(paths, texts))
    r = subprocess.run(base + ["--inputs", ",".join(paths), "--long", "--max-positions", str(bm.P), "--timestamps"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 105 and "--inputs requires --long --timestamps --seek" in r.stderr


def run_plain(eng, xs):
    try:
        return eng.transcribe_long_batch(xs)
    finally:
        restore(eng)
