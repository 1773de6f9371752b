"""The rest of the full-length chains in the bf16 storage mode (options bf16 + full_bf16 + full_bf16_all + max_positions,
DESIGN.md section 34) on the GPU: per-clip contexts and wt_transcribe_long_batch, language = -1 behind full_language,
and word_timestamps.

The oracle is fp32 and a bf16 engine may legitimately choose other ids, so, as in tests/test_gpu_full_bf16.py, the oracle
is teacher-forced along the engine's OWN ids and the reported token log-probabilities are held to bar_lp = 2 * (2 * E),
E measured when the module runs on the unchanged 31-position chain (bf16 logits behind forced fp32 ids against the fp32
engine).  Whatever is exact in fp32 because two paths run the same arithmetic is exact here too: equal contexts through
set_contexts against set_context, a detecting chain against the explicit language, the engine's loop against its own
windows, the discrete stages of the alignment against align_ref on the engine's own W and C.

The language section runs the comparisons of tests/test_gpu_full_language.py on bf16 engines, through a private copy of
that module whose engine factory makes bf16 engines (tests/full_bf16_all_util.py): behind either kind of context, the
fixture whose text follows the language, word timestamps per clip's language, both long calls — called as they stand —
and, restated here because they name fp32 literals or a fresh default engine, detection against detect_language on the
same engine, automatic against explicit in every mode, graphs eager / replayed / on other audio / use_graphs 0, every
entry of WIDE, candidate lists (the detect_language halves included) and task = 1.  Left out, each for its reason:
  * the oracle's greedy ROWS (ref["rows"], exact in fp32 because every margin exceeds 2e-4) and the log-probabilities
    against the oracle at TOKEN_BOUND: a bf16 engine may choose other ids and differs by E, not by 1e-4; in their place
    the path consistency behind each clip's detected language at bar_lp;
  * the 31-position and pipelined halves of its candidates and task tests (max_positions = 0): not this option's code,
    the parent runs them in bf16 as it did;
  * its refusal test: the fp32 engine's refusals; this option's are test_the_option_at_0_keeps_every_refusal;
  * behind beam search and best_of the reported probability is held to detect_language on the SAME engine, not to a
    fresh default engine: those chains detect on the absorbed cross-attention, a fresh engine detects four clips on the
    cached form, and in bf16 the two forms round different operands (3e-3 apart; 1e-6 in fp32).

Without the feature set_option("full_bf16_all", 1) fails and so does every test here."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import align_ref  # noqa: E402
import full_language_model as flm  # noqa: E402
import lang_model as lgm  # noqa: E402
import longform_batch_model as bm  # noqa: E402
import longform_model as lm  # noqa: E402
import longform_ref as lr  # noqa: E402
import full_bf16_all_util as util  # noqa: E402
import ts_model as tm  # noqa: E402
import ts_ref  # noqa: E402

# private copies (full_bf16_all_util.private_copy): module objects of this file's own, not the ones pytest collects
fb = util.private_copy("test_gpu_full_bf16")        # Oracle, check_path, decode, status_of
fl = util.private_copy("test_gpu_full_language")    # its comparisons, run on bf16 engines:
fl.new_engine = util.bf16_engine_factory(fl.new_engine, fl.P)  # every engine its functions make is a bf16 engine
tw = util.private_copy("test_gpu_word_timestamps")  # decode, long_call, check_windows, pcm_clip

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
PREV = 50361
P_CTX = 78                     # 11 positions behind the longest fed prompt (63 context ids kept of 200)
KEEP = tm.N_TEXT_CTX // 2 - 1
LENGTHS = (0, 3, 27, 200)      # context lengths of one call, cycled over its clips
C_BOUND = tw.C_BOUND
status_of = fb.status_of


@pytest.fixture(scope="module")
def files(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    d = tmp_path_factory.mktemp("fullbf16all")
    out = {k: (str(d / ("micro-" + k)), vocab) for k in ("ts", "long", "fa")}
    tm.write_model(prefix + ".wtw", out["ts"][0] + ".wtw")
    lm.write_model(prefix + ".wtw", out["long"][0] + ".wtw")
    flm.write_a(prefix + ".wtw", out["fa"][0] + ".wtw")
    return out


@pytest.fixture(scope="module")
def mels():
    out = {"ts": tm.mels(32), "fa": np.ascontiguousarray(lgm.lang_mels()[list(flm.CLIPS)])}
    out["long"] = out["ts"]  # (the seeking model's E is measured on the same clips; its tests decode their own audio)
    for m in out.values():
        m.setflags(write=False)
    return out


def new_engine(pkg, files, model, bf16=True, positions=None, **options):
    eng = pkg.Engine(files[model][0], files[model][1], True)
    if positions:
        eng.set_option("max_positions", positions)
    if model != "fa":
        eng.set_option("timestamps", 1)
    eng.set_option("scores", 1)
    if bf16:
        for k in ("bf16", "full_bf16", "full_bf16_all"):
            eng.set_option(k, 1)
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


@pytest.fixture(scope="module")
def bars(pkg, files, mels):
    """Per model E and bar_lp = 4 E, from the 31-position chain: bf16 logits behind forced fp32 ids against fp32 logits
    (the measurement of tests/test_gpu_full_bf16.py; the code it runs is not this option's)."""
    out = {}
    for model in ("ts", "long", "fa"):
        e = pkg.Engine(files[model][0], files[model][1], True)
        e.set_option("stop_at_eot", 0)
        mel = np.ascontiguousarray(mels[model][:4])
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
        print(f"[full_bf16_all] model {model}: E = {E:.4e}, bar_lp = {4 * E:.4e}")
    return out


@pytest.fixture(scope="module")
def oracle(orc, files, mels):
    o = fb.Oracle(orc, files, mels)
    yield o
    o.close()


def context(n):
    rng = np.random.default_rng(100 + n)
    return [int(i) for i in rng.integers(0, tm.EOT, size=n)]


def fed(n_ctx):
    ctx = context(n_ctx)
    return ([PREV] + ctx[-KEEP:] if ctx else []) + list(tm.PROMPT)


def layout(batch):
    """(clip, context length) of every row: the lengths cycled over two distinct clips (every length behind either)."""
    return [((b // len(LENGTHS)) % 2, LENGTHS[b % len(LENGTHS)]) for b in range(batch)]


forced = {}  # (clip, context length, ids) -> largest |lp - teacher-forced lp|: the oracle runs once per distinct row


def decode_rows(eng, mel, rows):
    eng.set_contexts([context(n) for _, n in rows])
    return fb.decode(eng, mel[[c for c, _ in rows]])


def check_rows(oracle, bars, what, got, rows):
    """Every row teacher-forced behind its OWN fed prompt."""
    ids, n, lp = got
    worst = 0.0
    for row, (clip, n_ctx) in enumerate(rows):
        prompt = fed(n_ctx)
        assert [int(x) for x in ids[row, : len(prompt)]] == prompt, (row, "the fed prompt")
        assert not lp[row, : len(prompt)].any()
        key = (clip, n_ctx, ids[row].tobytes(), lp[row].tobytes())
        if key not in forced:  # (equal ids and equal reported values: the same comparison)
            forced[key] = fb.check_path(oracle, bars, "ts", f"{what} row {row}", (ids[row:row + 1], n[row:row + 1], lp[row:row + 1]),
                                        len(prompt), P_CTX, True, clips=[clip])
        worst = max(worst, forced[key])
    print(f"[full_bf16_all] {what}: largest |lp - teacher-forced lp| {worst:.4e} (bar_lp {bars['ts']['bar_lp']:.4e})")


# ------------------------------------------------------------------------------------------- the option at 0 ---
def test_the_option_at_0_keeps_every_refusal(pkg, files, mels):
    e = new_engine(pkg, files, "ts", positions=P_CTX)
    e.set_option("full_bf16_all", 0)
    assert e.get_option("full_bf16_all") == 0
    mel = np.ascontiguousarray(mels["ts"][:2])
    want = e.encdec_tokens_full(mel)

    def refused(fn, word="full_bf16"):
        with pytest.raises(pkg.WtError) as x:
            fn()
        assert status_of(x) == UNSUPPORTED and word in str(x.value), str(x.value)

    run = lambda: e.encdec_tokens_full(mel)  # noqa: E731
    pcm = np.zeros(e.pcm_len, np.float32)
    language = e.get_option("language")

    def all_three():
        e.set_option("word_timestamps", 1)
        refused(run)
        e.set_option("word_timestamps", 0)
        e.set_contexts([[1, 2, 3], []])
        refused(run)
        e.set_contexts([])
        e.set_option("language", -1)
        e.set_option("full_language", 1)
        refused(run)
        e.set_option("full_language", 0)
        e.set_option("language", language)
        e.set_option("seek", 1)
        refused(lambda: e.transcribe_long_batch([pcm, pcm]))
        e.set_option("seek", 0)

    all_three()
    for bad in (-1, 2):
        with pytest.raises(pkg.WtError) as x:
            e.set_option("full_bf16_all", bad)
        assert status_of(x) == INVALID
    assert e.get_option("full_bf16_all") == 0
    got = e.encdec_tokens_full(mel)  # after every refusal a default transcription works
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the option means nothing without full_bf16, and the standing cuts of other options keep their own texts
    e.set_option("full_bf16_all", 1)
    e.set_option("full_bf16", 0)
    refused(run, "full_bf16")
    e.set_option("full_bf16", 1)
    e.set_contexts([[1, 2, 3], []])
    e.set_option("word_timestamps", 1)
    refused(run, "contexts")
    e.set_option("word_timestamps", 0)
    e.set_option("beam_size", 2)
    e.set_option("full_beam", 1)
    refused(run, "full_beam")
    e.set_option("beam_size", 1)
    e.set_contexts([])
    e.set_option("seek", 1)
    e.set_option("temperature", 600)
    e.set_option("best_of", 2)
    refused(lambda: e.transcribe_long_batch([pcm, pcm]), "best_of")
    e.set_option("best_of", 1)
    e.set_option("temperature", 0)
    e.set_option("seek", 0)
    got = e.encdec_tokens_full(mel)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    e.close()


# --------------------------------------------------------------------------------------------------- contexts ---
@pytest.mark.parametrize("batch", [5, 32])
def test_contexts_every_clip_behind_its_own_prompt(pkg, files, mels, oracle, bars, batch):
    """5 clips: the cached cross-attention; 32: the absorbed one."""
    eng = new_engine(pkg, files, "ts", positions=P_CTX)
    rows = layout(batch)
    got = decode_rows(eng, mels["ts"], rows)
    check_rows(oracle, bars, f"contexts, {batch} clips", got, rows)
    again = decode_rows(eng, mels["ts"], rows)
    assert np.array_equal(again[0], got[0]) and again[2].tobytes() == got[2].tobytes()
    eng.close()


def test_equal_contexts_are_the_set_context_path(pkg, files, mels):
    """The ragged bf16 kernels carry the unragged ones' bits at every clip's own position, so the ids are the same: a
    difference here is a finding, not rounding."""
    eng = new_engine(pkg, files, "ts", positions=P_CTX)
    for batch in (5, 32):
        mel = np.ascontiguousarray(mels["ts"][[b % 4 for b in range(batch)]])
        for n_ctx in (27, 200):
            eng.set_contexts([context(n_ctx)] * batch)
            ids, n = eng.encdec_tokens_full(mel)
            eng.set_context(context(n_ctx))
            assert eng.get_option("context_clips") == 0
            ids1, n1 = eng.encdec_tokens_full(mel)
            assert np.array_equal(ids, ids1) and np.array_equal(n, n1), (batch, n_ctx)
            eng.set_context([])
    eng.close()


def test_contexts_sampling_clearing_and_graphs(pkg, files, mels, oracle, bars):
    rows = layout(5)
    eng = new_engine(pkg, files, "ts", positions=P_CTX, temperature=600, seed=7)
    got = decode_rows(eng, mels["ts"], rows)
    check_rows(oracle, bars, "contexts, sampling T 0.6", got, rows)
    again = decode_rows(eng, mels["ts"], rows)  # same audio, options and seed: the same ids
    assert np.array_equal(again[0], got[0]) and again[2].tobytes() == got[2].tobytes()
    eng.close()
    # clearing the contexts restores the ids of an engine that never had the option, and the graphs are untouched
    three = np.ascontiguousarray(mels["ts"][:3])
    parent = new_engine(pkg, files, "ts", positions=P_CTX, full_bf16_all=0)
    want = fb.decode(parent, three)
    parent.close()
    eng = new_engine(pkg, files, "ts", positions=P_CTX)
    first = fb.decode(eng, three)
    held = eng.get_option("graphs_cached")
    assert held >= 1
    for lengths in ((0, 1, 2), (5, 0, 63), (27, 27, 3), (0, 0, 0)):
        eng.set_contexts([context(k) for k in lengths])
        eng.encdec_tokens_full(three)
        assert eng.get_option("graphs_cached") == held, lengths
    eng.set_contexts([])
    back = fb.decode(eng, three)
    assert eng.get_option("graphs_cached") == held
    for a in (first, back):
        assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1]) and a[2].tobytes() == want[2].tobytes()
    eng.close()


# ------------------------------------------------------------------------------------- transcribe_long_batch ---
def long_engine(pkg, files):
    e = new_engine(pkg, files, "long", positions=bm.P)
    e.set_option("no_speech_threshold", lm.NO_SPEECH_THRESHOLD)
    e.set_option("logprob_threshold", lm.LOGPROB_THRESHOLD)
    e.set_option("skip_silence", 1)
    return e


class Stop(Exception):
    pass


def replay(eng, audio, decode_round):
    """longform_ref's loop per file over windows decoded round by round: round w holds window w of every file that has
    one, decoded by decode_round(w, [(file, seek, fed)]) -> one record per entry.  Returns the files' window lists."""
    done, cache, w = {}, {f: [] for f in range(len(audio))}, 0
    while len(done) < len(audio):
        asked = []
        for f in range(len(audio)):
            if f in done:
                continue

            def dec(k, seek, fed_ids, f=f):
                if k < len(cache[f]):
                    return cache[f][k]
                asked.append((f, seek, [int(i) for i in fed_ids]))
                raise Stop()

            try:
                done[f] = lr.transcribe(dec, audio[f].size, bm.WIN, lm.EOT, lm.BEG, lm.PREV, lm.PROMPT, bm.KEEP)
            except Stop:
                pass
        if asked:
            for (f, _, _), rec in zip(asked, decode_round(w, asked)):
                cache[f].append(rec)
        w += 1
    return [done[f] for f in range(len(audio))]


def window_records(eng, ids, n, fed_list):
    lp, sc = eng.last_token_logprobs(bm.P + 1), eng.last_scores()
    out = []
    for b, fed_ids in enumerate(fed_list):
        row = [int(x) for x in ids[b, : n[b]]]
        assert row[: len(fed_ids)] == fed_ids  # the prompt the loop hands over is the prefix of the recorded ids
        out.append({"ids": row, "lp": lp[b].copy(), "skipped": bool(sc["skipped"][b])})
    return out


@pytest.fixture(scope="module")
def long_batch(pkg, files):
    """The engine's part of the batched seeking tests, once: the reference loop over the engine's own round decodes, the
    batch call itself, and every file alone (the loop over single-window decodes, and transcribe_long).

    A deliberate choice: the library hands out no id rows of a long call's windows (wt_last_windows, wt_last_segments and
    wt_last_token_logprobs only), so "the batch call's own recorded ids" are obtained by decoding every round once more
    through the public calls the batch loop is defined by (wt_engine_set_contexts + one full-length call per round, the
    same clips in the same order).  That is a second run, deterministic and identical to the call's by construction; the
    loop-consistency test holds the call's reported windows to it, and the path-consistency test holds the call's REPORTED
    log-probabilities to the oracle along these ids, so ids that were not the call's would show there as errors far
    above rounding.  Should the two runs ever stop being identical, both tests fail and the cause is this replay or the
    loop's round composition, not the kernels."""
    eng = long_engine(pkg, files)
    audio = [bm.pcm(f) for f in range(len(bm.FILES))]
    n_tail = len(lm.PROMPT)
    mel_of = {}

    def ctx_of(fed_ids):
        return fed_ids[1: len(fed_ids) - n_tail] if len(fed_ids) > n_tail else []

    def batch_round(w, asked):  # one window of every running file as ONE batch behind per-clip contexts: the call's round
        mel = np.concatenate([eng.logmel_batch(lm.window(audio[f], seek)) for f, seek, _ in asked])
        for (f, seek, _), m in zip(asked, mel):
            mel_of[(f, seek)] = m
        eng.set_contexts([ctx_of(fd) for _, _, fd in asked])
        ids, n = eng.encdec_tokens_full(mel)
        return window_records(eng, ids, n, [fd for _, _, fd in asked])

    def alone_round(w, asked):  # a file alone: one window behind set_context, as the seeking transcribe_long decodes it
        (f, seek, fd), = asked
        eng.set_context(ctx_of(fd))
        ids, n = eng.encdec_tokens_full(eng.logmel_batch(lm.window(audio[f], seek)))
        return window_records(eng, ids, n, [fd])

    out = {"audio": audio, "mel_of": mel_of, "runs": replay(eng, audio, batch_round)}
    eng.set_contexts([])
    out["texts"] = eng.transcribe_long_batch(audio)
    out["win"], out["wf"], out["lp"] = eng.last_windows(), eng.last_window_files(), eng.last_token_logprobs(bm.P + 1)
    out["alone"], out["alone_text"] = [], []
    for f in range(len(audio)):
        out["alone"].append(replay(eng, [audio[f]], lambda w, asked, f=f: alone_round(w, [(f, asked[0][1], asked[0][2])]))[0])
        eng.set_context([])
        eng.set_option("seek", 1)
        out["alone_text"].append(eng.transcribe_long(audio[f]))
        eng.set_option("seek", 0)
    out["one"] = (eng.transcribe_long_batch([audio[2]]), eng.last_window_files())  # one file through the batch call
    out["line"] = lambda kept: eng.decode_text(np.asarray(kept, np.int64))
    yield out
    eng.close()


def test_transcribe_long_batch_loop_consistency(long_batch):
    """The call reports the windows the reference loop makes of the call's own ids."""
    runs, win, wf, lp = long_batch["runs"], long_batch["win"], long_batch["wf"], long_batch["lp"]
    flat = [(f, r) for f, ws in enumerate(runs) for r in ws]
    assert win.size == len(flat) == wf.size and [int(x) for x in wf] == [f for f, _ in flat]
    assert any(r["n_context"] > 0 for _, r in flat) and len({r["n_prompt"] for _, r in flat}) >= 3
    for i, (f, r) in enumerate(flat):
        w = win[i]
        assert (int(w["seek_sample"]), int(w["advance_samples"]), int(w["n_context"]), int(w["n_prompt"]), int(w["n_kept_ids"]),
                int(w["skipped"])) == (r["seek"], r["advance"], r["n_context"], r["n_prompt"], len(r["kept"]), int(r["skipped"])), (f, i)
        assert not lp[i, :r["n_prompt"]].any() and not lp[i, len(r["ids"]):].any(), (f, i)
    for f, ws in enumerate(runs):
        assert long_batch["texts"][f].split("\n") == [long_batch["line"](r["kept"]) for r in ws], f
    one, one_files = long_batch["one"]
    assert one == [long_batch["alone_text"][2]] and not one_files.any()


@pytest.mark.parametrize("f", range(len(bm.FILES)))
def test_transcribe_long_batch_file(long_batch, oracle, bars, f):
    """Path consistency: every window's REPORTED log-probabilities, teacher-forced behind its fed prompt.  Batch against
    alone: up to the first differing id, which must lie inside the oracle's 2 E margin (section 4.2's rule)."""
    runs, wf, lp, mel_of = long_batch["runs"], long_batch["wf"], long_batch["lp"], long_batch["mel_of"]
    rows = np.nonzero(wf == f)[0]
    assert rows.size == len(runs[f])
    worst = 0.0
    for i, r in zip(rows, runs[f]):
        n0, ids = r["n_prompt"], r["ids"]
        want = np.asarray(oracle.token_logprobs("long", ("batch", f, r["seek"]), ids, n0, bm.P, True, mel=mel_of[(f, r["seek"])]), np.float64)
        assert np.isfinite(want).all(), (f, i)
        worst = max(worst, float(np.abs(lp[i, n0: len(ids)].astype(np.float64) - want).max()))
    print(f"[full_bf16_all] transcribe_long_batch file {f}: {rows.size} windows, largest |lp - teacher-forced lp| {worst:.4e} "
          f"(bar_lp {bars['long']['bar_lp']:.4e}, E {bars['long']['E']:.4e})")
    assert worst <= bars["long"]["bar_lp"]
    alone = long_batch["alone"][f]
    assert long_batch["alone_text"][f].split("\n") == [long_batch["line"](r["kept"]) for r in alone], f
    differed = 0
    for k, (a, b) in enumerate(zip(runs[f], alone)):
        if a["ids"] == b["ids"]:
            assert (a["seek"], a["advance"], a["n_prompt"], a["kept"]) == (b["seek"], b["advance"], b["n_prompt"], b["kept"])
            continue
        differed = 1
        assert (a["seek"], a["n_prompt"]) == (b["seek"], b["n_prompt"]), (f, k)
        at = next(i for i, (x, y) in enumerate(zip(a["ids"], b["ids"])) if x != y)
        assert at >= a["n_prompt"], (f, k)
        fn = oracle.logits_fn("long", ("batch", f, a["seek"]), bm.P, mel_of[(f, a["seek"])])
        _, info = ts_ref.step(np.asarray(fn(a["ids"][:at]), np.float32), a["ids"][a["n_prompt"]:at], lm.EOT, lm.BEG)
        margin = min(info["gap_lm"], info["gap_top"])
        print(f"[full_bf16_all] file {f} window {k}: batch and alone part at id {at}, oracle margin {margin:.3e}")
        assert margin <= 2 * bars["long"]["E"], (f, k, at, margin)
        break
    else:
        assert len(runs[f]) == len(alone)
    print(f"[full_bf16_all] batch against alone, file {f}: {'differed' if differed else 'the same ids in every window'}")


def test_the_cli_prints_every_file(pkg, files, tmp_path):
    exe = os.path.join(ROOT, "whisper.tflite_amd", "bin", "encdec")
    paths, xs = [], []
    for f in (1, 2):
        pcm16 = np.clip(np.round(bm.pcm(f)[: 2 * bm.WIN + 5000] * 32767), -32768, 32767).astype("<i2")
        wav = tmp_path / ("f%d.wav" % f)
        wav.write_bytes(b"RIFF" + struct.pack("<I", 36 + pcm16.nbytes) + b"WAVEfmt " +
                        struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" +
                        struct.pack("<I", pcm16.nbytes) + pcm16.tobytes())
        paths.append(str(wav))
        xs.append(pkg.wav_read_legacy(str(wav)))
    eng = new_engine(pkg, files, "long", positions=bm.P, scores=0)
    texts = eng.transcribe_long_batch(xs)
    eng.close()
    r = subprocess.run([exe, "--model-prefix", files["long"][0], "--vocab", files["long"][1], "--bf16", "--inputs", ",".join(paths),
                        "--long", "--timestamps", "--seek", "--max-positions", str(bm.P)],
                       capture_output=True, text=True, errors="replace", timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "".join("== %s\n%s\n" % (p, t) for p, t in zip(paths, texts))


def write_wav(path, pcm):
    pcm16 = np.clip(np.round(pcm * 32767), -32768, 32767).astype("<i2")
    path.write_bytes(b"RIFF" + struct.pack("<I", 36 + pcm16.nbytes) + b"WAVEfmt " +
                     struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" + struct.pack("<I", pcm16.nbytes) + pcm16.tobytes())
    return str(path)


def test_the_cli_forms_lang_auto_and_word_timestamps(pkg, files, tmp_path):
    """encdec --bf16 --max-positions N with --lang auto, and with --word-timestamps: both set full_bf16_all (without it the
    library refuses the call) and print what the library gives for the same file and options."""
    exe = os.path.join(ROOT, "whisper.tflite_amd", "bin", "encdec")
    wav = write_wav(tmp_path / "clip.wav", tw.pcm_clip(1, 32000))
    # --lang auto
    e = new_engine(pkg, files, "fa", positions=fl.P, scores=0, full_language=1, language=-1)
    text = e.transcribe(wav)
    lang, _ = e.last_languages()
    e.close()
    r = subprocess.run([exe, "--model-prefix", files["fa"][0], "--vocab", files["fa"][1], "--input", wav, "--bf16", "--lang", "auto",
                        "--max-positions", str(fl.P)], capture_output=True, text=True, errors="replace", timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[-1] == "" and lines[-2] == text
    assert sum(1 for ln in lines if ln.startswith("language: ")) == 1 and lang.size == 1
    # --word-timestamps
    e = new_engine(pkg, files, "ts", positions=tm.P_SHORT, scores=0, word_timestamps=1)
    e.transcribe(wav)
    words, texts = e.last_words(with_text=True)
    e.close()
    r = subprocess.run([exe, "--model-prefix", files["ts"][0], "--vocab", files["ts"][1], "--input", wav, "--bf16", "--timestamps",
                        "--word-timestamps", "--max-positions", str(tm.P_SHORT)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = [b"%.2f %.2f " % (w["t0_ms"] / 1000.0, w["t1_ms"] / 1000.0) + t for w, t in zip(words, texts)]
    assert words.size > 0 and r.stdout.split(b"\n")[-1 - len(want):-1] == want


# --------------------------------------------------------------------------------------------------- language ---
@pytest.fixture(scope="module")
def bf16_language_engines(pkg, files, mels):
    """The language fixture A; the copy's LANGS become what a bf16 engine detects on the four clips (asserted to be the
    fp32 values' set: the comparisons taken over hold each clip to ITS language, whichever it is)."""
    e = pkg.Engine(*files["fa"], True)
    e.set_option("bf16", 1)
    lang = [int(x) for x in e.detect_language(mels["fa"])[0]]
    e.close()
    assert set(lang) == {87, 94}, lang
    fl.LANGS = lang
    return files["fa"]


@pytest.fixture(scope="module")
def detected(pkg, bf16_language_engines, mels):
    e = pkg.Engine(*bf16_language_engines, True)
    e.set_option("bf16", 1)
    out = e.detect_language(mels["fa"])
    e.close()
    return out


def test_language_detection_is_the_detect_call(pkg, bf16_language_engines, mels, detected, oracle, bars):
    fix, mel = bf16_language_engines, mels["fa"]
    e = fl.new_engine(pkg, fix, scores=1)
    assert (e.get_option("bf16"), e.get_option("full_bf16_all"), e.get_option("full_language")) == (1, 1, 1)
    ids, n = e.encdec_tokens_full(mel)
    lp = e.last_token_logprobs(ids.shape[1])
    lang, prob = e.last_languages()
    same = e.detect_language(mel)  # on the same engine
    e.close()
    assert np.array_equal(lang, detected[0]) and np.array_equal(lang, same[0])
    for i in range(4):
        assert abs(float(prob[i]) - float(same[1][i, lang[i]])) <= fl.P_TOL
    assert np.array_equal(ids[:, 1], lgm.LANG_LO + lang.astype(np.int64))
    assert np.all(ids[:, 0] == lgm.SOT) and np.all(ids[:, 2] == lgm.TRANSCRIBE) and np.all(ids[:, 3] == lgm.NOTIMESTAMPS)
    # path consistency behind each clip's own detected language
    for i in range(4):
        fb.check_path(oracle, bars, "fa", f"automatic language clip {i}", (ids[i:i + 1], n[i:i + 1], lp[i:i + 1]), 4, fl.P, False,
                      clips=[i])


@pytest.mark.parametrize("mode", list(fl.MODES))
def test_language_automatic_equals_explicit(pkg, bf16_language_engines, mels, detected, mode):
    fix, mel, opts = bf16_language_engines, mels["fa"], fl.MODES[mode]
    e = fl.new_engine(pkg, fix, **opts)
    ids, n = e.encdec_tokens_full(mel)
    lang, _ = e.last_languages()
    segs = e.last_segments() if opts.get("timestamps") else None
    lps = e.last_token_logprobs(ids.shape[1]) if opts.get("scores") else None
    e.close()
    assert np.array_equal(lang, detected[0])
    want = fl.explicit_rows(pkg, fix, mel, lang, **opts)
    for i in range(4):
        w = want[int(lang[i])]
        assert np.array_equal(ids[i], w[0][i]) and n[i] == w[1][i], (mode, i)
        if segs is not None:
            assert np.array_equal(segs[segs["clip"] == i], w[2][w[2]["clip"] == i])
        if lps is not None:
            assert np.array_equal(lps[i], w[3][i])


@pytest.mark.parametrize("kind", ["context", "ragged"])
@pytest.mark.parametrize("mode", ["plain", "scores"])
def test_language_behind_a_context(pkg, bf16_language_engines, mels, kind, mode):
    fl.test_behind_a_context(pkg, bf16_language_engines, mels["fa"], kind, mode)


def test_language_graphs_eager_and_replay_on_other_audio(pkg, bf16_language_engines, mels):
    """fl.test_graphs_eager_and_replay_on_other_audio with the languages a bf16 engine detects in place of the literals:
    the detecting chain's graphs (key entry in front of kBf16KeyMark) eager, captured, replayed on the same audio and on
    other audio, and use_graphs = 0."""
    fix, mel = bf16_language_engines, mels["fa"]
    order = [1, 0, 3, 2]  # the same clips in another order: other languages per row
    other = np.ascontiguousarray(mel[order])
    e = fl.new_engine(pkg, fix)
    a = e.encdec_tokens_full(mel)     # eager, then captured
    lang_a, _ = e.last_languages()
    held = e.get_option("graphs_cached")
    b = e.encdec_tokens_full(mel)     # replayed
    c = e.encdec_tokens_full(other)   # replayed on other audio: that audio's languages
    lang_c, _ = e.last_languages()
    assert held >= 1 and e.get_option("graphs_cached") == held
    e.set_option("use_graphs", 0)
    d = e.encdec_tokens_full(mel)
    lang_d, _ = e.last_languages()
    e.close()
    assert list(lang_a) == fl.LANGS == list(lang_d) and list(lang_c) == [fl.LANGS[k] for k in order]
    assert list(lang_c) != list(lang_a)
    for x in (b, d):
        assert np.array_equal(x[0], a[0]) and np.array_equal(x[1], a[1])
    for row, k in enumerate(order):  # every clip's row, wherever it sits
        assert np.array_equal(c[0][row], a[0][k]) and c[1][row] == a[1][k], (row, k)
    f = fl.new_engine(pkg, fix, full_bf16_all=1)  # and not the fp32 engine's graphs: a fresh fp32 engine gives other values
    f.set_option("bf16", 0)
    f.set_option("scores", 1)
    f.encdec_tokens_full(mel)
    lp32 = f.last_token_logprobs(fl.P + 1)
    f.set_option("bf16", 1)
    f.encdec_tokens_full(mel)
    lp16 = f.last_token_logprobs(fl.P + 1)
    f.close()
    assert not np.array_equal(lp32, lp16)


def test_language_fixture_b_text_follows_the_detected_language(pkg, files, assets, tmp_path):
    prefix, vocab = assets("micro")
    p = str(tmp_path / "micro-flang-b")
    flm.write_b(prefix + ".wtw", p + ".wtw")
    fl.test_fixture_b_text_follows_the_detected_language(pkg, (p, vocab))


def test_language_word_timestamps_follow_each_clips_language(pkg, bf16_language_engines, mels, tmp_path):
    """Automatic language and word_timestamps together: the alignment rows carry the clip's own language token under the
    bf16 pass, and the word-splitting rule follows the clip's language."""
    word_vocab = str(tmp_path / "word_vocab.bin")
    flm.write_word_vocab(bf16_language_engines[1], word_vocab)
    fl.test_word_timestamps_follow_each_clips_language(pkg, bf16_language_engines, word_vocab, mels["fa"])


@pytest.mark.parametrize("mode", list(fl.WIDE))
def test_language_behind_beam_search_and_best_of(pkg, bf16_language_engines, mels, detected, mode):
    """fl.test_beam_and_best_of_carry_each_clips_language against detect_language on the SAME engine: these chains run the
    absorbed cross-attention whatever the batch, and so does a detection on an engine with their options, while a fresh
    engine detects four clips on the cached form — in the bf16 storage mode the two forms round different operands, so
    their probabilities agree to the mode's rounding only (3e-3 here), not to the 1e-6 of one form against itself."""
    fix, mel = bf16_language_engines, mels["fa"]
    opts = fl.WIDE[mode]
    if "best_of" in opts:
        opts = dict(opts, cross_absorb=1)
    e = fl.new_engine(pkg, fix, **opts)
    ids, n = e.encdec_tokens_full(mel)
    lang, prob = e.last_languages()
    info = e.last_decode_info() if "temperature_fallback" in opts else None
    same = e.detect_language(mel)
    e.close()
    assert np.array_equal(lang, same[0]) and np.array_equal(lang, detected[0])  # detection runs per clip, not per hypothesis
    assert np.abs(prob - same[1][np.arange(4), lang]).max() <= 1e-6
    assert np.array_equal(ids[:, 1], lgm.LANG_LO + lang.astype(np.int64))
    want = fl.explicit_rows(pkg, fix, mel, lang, **opts)
    for i in range(4):
        w = want[int(lang[i])]
        assert np.array_equal(ids[i], w[0][i]) and n[i] == w[1][i], (mode, i)
    if info is not None:
        print(mode, "attempts per clip:", info["attempts"].tolist())
        assert info["attempts"].min() > 1  # the attempts with best_of rows ran


def test_language_candidates_and_task(pkg, bf16_language_engines, mels, detected):
    fix, mel = bf16_language_engines, mels["fa"]
    e = fl.new_engine(pkg, fix)
    base = e.encdec_tokens_full(mel)
    assert e.get_option("language_candidates") == 0
    e.set_language_candidates([87, 87])  # duplicates count once
    assert e.get_option("language_candidates") == 1
    lang1, probs1 = e.detect_language(mel)  # the masked probabilities are exactly 1 and 0
    assert list(lang1) == [87] * 4 and np.all(probs1[:, 87] == 1.0) and np.all(np.delete(probs1, 87, axis=1) == 0.0)
    ids, n = e.encdec_tokens_full(mel)
    fl_, fp_ = e.last_languages()
    assert list(fl_) == [87] * 4 and np.all(fp_ == 1.0) and np.all(ids[:, 1] == lgm.LANG_LO + 87)
    want = fl.explicit_rows(pkg, fix, mel, [87])[87]
    assert np.array_equal(ids, want[0]) and np.array_equal(n, want[1])
    e.set_language_candidates([94, 87])
    assert e.get_option("language_candidates") == 2
    lang, probs = e.detect_language(mel)
    assert list(lang) == fl.LANGS
    for i in range(4):  # two candidates: the detected values renormalised
        p2 = detected[1][i].astype(np.float64)[[87, 94]]
        p2 /= p2.sum()
        assert np.abs(probs[i, [87, 94]] - p2).max() <= fl.P_TOL and probs[i].sum() == pytest.approx(1.0, abs=1e-5)
        assert np.all(np.delete(probs[i], [87, 94]) == 0.0)
    ids2, _ = e.encdec_tokens_full(mel)
    fl2, fp2 = e.last_languages()
    assert np.array_equal(fl2, lang) and np.abs(fp2 - probs[np.arange(4), fl2]).max() <= 1e-6
    assert np.array_equal(ids2[:, 1], lgm.LANG_LO + lang.astype(np.int64))
    e.set_language_candidates([])
    again = e.encdec_tokens_full(mel)
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1])
    e.set_option("task", 1)
    ids_t, n_t = e.encdec_tokens_full(mel)
    lang_t, _ = e.last_languages()
    e.close()
    assert np.array_equal(lang_t, detected[0]) and np.all(ids_t[:, 2] == flm.TRANSLATE)
    want = fl.explicit_rows(pkg, fix, mel, lang_t, task=1)
    for i in range(4):
        w = want[int(lang_t[i])]
        assert np.array_equal(ids_t[i], w[0][i]) and n_t[i] == w[1][i], i


@pytest.fixture(scope="module")
def language_files(pkg, bf16_language_engines):
    """fl.files on a bf16 engine: recordings of 2.5 windows whose first windows detect different languages."""
    e = pkg.Engine(*bf16_language_engines, True)
    e.set_option("bf16", 1)
    win = e.pcm_len
    pool = []
    for seed in range(6):
        for amp in (0.002, 0.02, 0.2, 1.0):
            x = fl.noise_pcm(seed, amp, win)
            pool.append((int(e.detect_language_pcm(x)[0]), x))
    e.close()
    langs = sorted(set(l for l, _ in pool))
    assert len(langs) >= 2, "the fixture needs windows of two languages"
    first = {L: next(x for l, x in pool if l == L) for L in langs[:2]}
    a, b = langs[:2]
    f0 = np.concatenate([first[a], first[b], first[a][: win // 2]])
    f1 = np.concatenate([first[b], first[b][::-1].copy(), first[b][: win // 2]])
    f2 = first[a][: win // 2].copy()
    return [f0, f1, f2], [a, b, None]


@pytest.mark.parametrize("seek", [0, 1])
def test_language_long_audio_holds_the_files_language(pkg, bf16_language_engines, language_files, seek):
    fl.test_long_audio_holds_the_files_language(pkg, bf16_language_engines, language_files, seek)


def test_language_batched_seek_holds_each_files_language(pkg, bf16_language_engines, language_files):
    fl.test_batched_seek_holds_each_files_language(pkg, bf16_language_engines, language_files)


# ------------------------------------------------------------------------------------------------------ words ---
@pytest.fixture(scope="module")
def word_engine(pkg, files):
    e = pkg.Engine(files["ts"][0], files["ts"][1], True)
    for k in ("bf16", "full_bf16", "full_bf16_all"):
        e.set_option(k, 1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def word_ref(pkg, files, mels):
    """The model's tensors and the fp32 engine's encoder output, for the float64 weights printed as information."""
    from wtw import read_wtw
    e = pkg.Engine(files["ts"][0], files["ts"][1], True)
    e.set_prompt([3, 5, 7, 11])
    _, _, enc, _ = e.encdec_debug_batch(mels["ts"], want_logits=False)
    e.close()
    return read_wtw(files["ts"][0] + ".wtw"), enc


info_w = {}


def check_words(pkg, eng, files, word_ref, ids, n, positions, what):
    """tests/test_gpu_word_timestamps.py's check_clips with the float64 weights as information only: they carry the
    bf16 decoder's and encoder's error, which nothing the parent can measure bounds.  Returns per clip (row, W, C, words)."""
    (dims, tensors), enc = word_ref
    vocab = pkg.Vocab(files["ts"][1], True)
    segs = eng.last_segments()
    words, texts = eng.last_words(with_text=True)
    lp = eng.last_token_logprobs(positions + 1)
    heads = sorted(align_ref.default_heads(dims))
    n_a, F = len(tm.PROMPT), dims["n_audio_ctx"]
    worst_w = worst_c = 0.0
    at_word, out = 0, []
    for b in range(ids.shape[0]):
        al = eng.dbg_last_alignment(b)
        row = [int(i) for i in ids[b, :n[b]]]
        where = [k for s in segs[segs["clip"] == b] for k in range(s["id_begin"], s["id_begin"] + s["id_count"]) if row[k] < tm.EOT]
        cap = dims["n_text_ctx"] - n_a - 2
        where = where[:cap]
        text = [row[k] for k in where]
        assert list(al["row"]) == tm.PROMPT + [tw.NOT] + text + [tm.EOT]
        assert (al["n_a"], al["L"], al["N"], al["F"], al["heads"]) == (n_a, n_a + len(text) + 2, len(text) + 1, F, len(heads))
        W = al["W"]
        assert np.all(W >= 0) and np.all(W[:, :, F:] == 0) and np.abs(W[:, :, :F].astype(np.float64).sum(axis=-1) - 1).max() <= 1e-5
        C64 = align_ref.cost_matrix(W, al["L"], F, n_a)  # the stage kernels on the engine's own W
        worst_c = max(worst_c, float(np.abs(al["C"][:, :F] - C64).max() / max(1.0, np.abs(C64).max())))
        jump = align_ref.dtw(al["C"][:, :F])[0]
        assert np.array_equal(al["jump"], jump), b
        W64 = align_ref.weights(dims, tensors, list(al["row"]), enc[b], heads, F)
        big = W64 > 1e-30
        worst_w = max(worst_w, float((np.abs(W - W64)[big] / W64[big]).max()))
        mine = words[words["clip"] == b]
        out.append((list(al["row"]), W.copy(), al["C"].copy(), mine.copy()))
        if not text:
            assert mine.size == 0
            continue
        toks = [vocab.token(i) for i in text + [tm.EOT]]
        want = align_ref.words(toks, text + [tm.EOT], tm.EOT, jump)
        assert mine.size == len(want), (b, mine, want)
        for w, (s0, cnt, t0, t1) in zip(mine, want):
            assert (w["t0_ms"], w["t1_ms"]) == (t0, t1)
            assert (w["id_begin"], w["id_count"]) == (where[s0], where[s0 + cnt - 1] - where[s0] + 1)
            seg = segs[w["segment"]]
            assert seg["clip"] == b and seg["id_begin"] <= w["id_begin"] < seg["id_begin"] + seg["id_count"]
            assert texts[at_word] == b"".join(toks[s0:s0 + cnt])
            p = float(np.mean(np.exp(lp[b, [where[s0 + k] for k in range(cnt)]].astype(np.float64))))
            assert abs(w["probability"] - p) <= 1e-6
            at_word += 1
    assert at_word == words.size
    vocab.close()
    info_w[what] = worst_w
    print(f"[full_bf16_all] words {what}: C err {worst_c:.3g} (bar {C_BOUND:.3g}), {words.size} words; information, no bar: "
          f"W against float64 along the engine's ids, relative {worst_w:.3g}")
    assert worst_c <= C_BOUND
    return out


@pytest.mark.parametrize("batch", [1, 5, 32])
@pytest.mark.parametrize("positions", [tm.P_SHORT, tm.P_LONG])
def test_words(pkg, word_engine, files, mels, word_ref, positions, batch):
    """Batches 1 and 5 decode on the cached cross-attention (the bf16 plane of E is made by f32_to_bf16), 32 on the
    absorbed one (the plane is the encoder's own)."""
    mel = np.ascontiguousarray(mels["ts"][:batch])
    ids, n = tw.decode(word_engine, mel, positions)
    got = check_words(pkg, word_engine, files, word_ref, ids, n, positions, f"P {positions} batch {batch}")
    if batch != 5:
        return
    for b in range(batch):  # a clip of the batch against the clip alone, wherever its ids are the same
        ids1, n1 = tw.decode(word_engine, mel[b:b + 1], positions)
        if not (n1[0] == n[b] and np.array_equal(ids1[0], ids[b])):
            print(f"[full_bf16_all] words: clip {b} alone chose other ids than in the batch of 5")
            continue
        al = word_engine.dbg_last_alignment(0)
        mine = word_engine.last_words()
        assert list(al["row"]) == got[b][0]
        assert np.array_equal(al["W"].view(np.uint32), got[b][1].view(np.uint32)), b
        assert np.array_equal(al["C"].view(np.uint32), got[b][2].view(np.uint32)), b
        want = got[b][3].copy()
        want["clip"] = 0
        want["segment"] -= want["segment"].min() if want.size else 0
        mine = mine.copy()
        mine["segment"] -= mine["segment"].min() if mine.size else 0
        assert mine.tobytes() == want.tobytes(), b


def test_words_other_forms_of_the_pass(pkg, word_engine, files, mels, word_ref):
    mel = np.ascontiguousarray(mels["ts"][:5])
    ids, n = tw.decode(word_engine, mel, tm.P_LONG)
    base = word_engine.last_words(with_text=True)
    for mode, sub in ((0, 0), (1, 1), (0, 1)):
        ids2, n2 = tw.decode(word_engine, mel, tm.P_LONG, mode=mode, sub=sub)
        assert np.array_equal(ids2, ids) and np.array_equal(n2, n)
        check_words(pkg, word_engine, files, word_ref, ids2, n2, tm.P_LONG, f"mode {mode} sub {sub}")
        other = word_engine.last_words(with_text=True)
        assert other[0].tobytes() == base[0].tobytes() and other[1] == base[1], (mode, sub)


def test_words_seeking_long_audio_numbers_the_windows(pkg, word_engine, files):
    win = 160 * word_engine.mel_shape[1]
    pcm = tw.pcm_clip(3, 3 * win + 4321)
    tw.long_call(word_engine, pcm, 1)
    wins = word_engine.last_windows()
    assert len(wins) >= 3
    frames = [min(100, max(1, min(win, pcm.size - int(w["seek_sample"])) // 320)) for w in wins]
    words = tw.check_windows(pkg, word_engine, files["ts"], len(wins), lambda w: int(wins[w]["seek_sample"]) // 16, frames)
    assert words.size > 0 and len(set(words["clip"].tolist())) >= 2


# ------------------------------------------------------------------------------------------------------- last ---
def test_switching_modes_on_one_engine_equals_fresh_engines(pkg, files, mels):
    """fp32 -> bf16 -> fp32 on one engine with each of the three features against engines that ran nothing else."""
    rows = layout(5)
    mel5 = np.ascontiguousarray(mels["ts"][[c for c, _ in rows]])

    def contexts(e):
        e.set_contexts([context(k) for _, k in rows])
        got = fb.decode(e, mel5)
        e.set_contexts([])
        return [got[0], got[1], got[2]]

    def words(e):
        e.set_option("word_timestamps", 1)
        got = fb.decode(e, mel5)
        w = e.last_words()
        e.set_option("word_timestamps", 0)
        return [got[0], got[1], got[2], w]

    def same(a, b):
        return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))

    for feature in (contexts, words):
        fresh = {}
        for bf in (0, 1):
            e = new_engine(pkg, files, "ts", bf16=bool(bf), positions=P_CTX)
            fresh[bf] = feature(e)
            e.close()
        e = new_engine(pkg, files, "ts", bf16=False, positions=P_CTX, full_bf16=1, full_bf16_all=1)
        for bf in (0, 1, 0):
            e.set_option("bf16", bf)
            assert same(feature(e), fresh[bf]), (feature.__name__, bf)
        e.close()
    # the language feature on its own model
    mel = mels["fa"]
    fresh = {}
    for bf in (0, 1):
        e = new_engine(pkg, files, "fa", bf16=bool(bf), positions=fl.P, full_language=1, language=-1)
        fresh[bf] = list(fb.decode(e, mel)) + list(e.last_languages())
        e.close()
    e = new_engine(pkg, files, "fa", bf16=False, positions=fl.P, full_bf16=1, full_bf16_all=1, full_language=1, language=-1)
    for bf in (0, 1, 0):
        e.set_option("bf16", bf)
        assert same(list(fb.decode(e, mel)) + list(e.last_languages()), fresh[bf]), bf
    e.close()


def test_zz_report(bars):
    for (model, what), worst in sorted(fb.observed.items()):
        if model in bars:
            print(f"[full_bf16_all] {model:5s} {what:44s} {worst:.4e}  (E {bars[model]['E']:.4e}, bar_lp {bars[model]['bar_lp']:.4e})")
    for what, w in sorted(info_w.items()):
        print(f"[full_bf16_all] words {what:24s} W against float64 (information): {w:.3e}")
