"""Automatic language behind max_positions (options full_language and task, wt_engine_set_language_candidates; DESIGN.md
section 32) on the GPU, against the CPU oracle behind each clip's own prompt and against fresh engines with the language
set explicitly, on the fixtures of tests/full_language_model.py (tests/test_full_language_reference.py pins them).
Without the feature the options and the function do not exist, so every test here fails."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import full_language_model as flm  # noqa: E402
import lang_model as lm  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
P = 48
P_TOL = 3e-4          # tests/test_gpu_language.py: a language probability under the project's logits bar
TOKEN_BOUND = 5 * 2.19e-5  # tests/test_gpu_scores.py: a token log-probability against the oracle
CLIPS = list(flm.CLIPS)
LANGS = [87, 94, 94, 87]


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def fix_a(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("flang") / "micro-flang-a")
    flm.write_a(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def fix_b(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("flang") / "micro-flang-b")
    flm.write_b(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def mel():
    m = np.ascontiguousarray(lm.lang_mels()[CLIPS])
    m.setflags(write=False)
    return m


@pytest.fixture(scope="module")
def ref(orc, fix_a, mel):
    """The oracle over the four clips, once: language logits, and per task the greedy rows at 48 and 30 positions with
    their margins and the log-probabilities of the generated ids under the whole vocabulary."""
    model = orc.Model(fix_a[0] + ".wtw")
    out = {"z": [], "rows": {}, "lp": []}
    for i in range(len(CLIPS)):
        enc = model.encode(mel[i])
        z, lang, gap = lm.oracle_language(model, enc)
        assert lang == LANGS[i] and gap > 0.05
        out["z"].append(z)
        for task in (lm.TRANSCRIBE, flm.TRANSLATE):
            for positions in (P, 30):
                ids, margin, _ = flm.decode(model, enc, flm.prompt_for(lang, task), positions)
                assert margin > 2e-4  # every step decisive: the rows are compared exactly
                out["rows"][(i, task, positions)] = ids
        ids, logits = model.decode_greedy(enc, flm.prompt_for(lang), P, lm.EOT, True, True, 8, True)
        zz = logits.astype(np.float64)
        lse = zz.max(axis=1) + np.log(np.exp(zz - zz.max(axis=1, keepdims=True)).sum(axis=1))
        out["lp"].append(np.array([zz[s, int(ids[4 + s])] - lse[s] for s in range(len(ids) - 4)]))
    model.close()
    return out


def new_engine(pkg, fix, language=-1, positions=P, **opts):
    e = pkg.Engine(fix[0], fix[1], True)
    e.set_option("max_positions", positions)
    for k, v in opts.items():
        e.set_option(k, v)
    if language < 0:
        e.set_option("full_language", 1)
    e.set_option("language", language)
    return e


def explicit_rows(pkg, fix, mel, langs, call=None, **opts):
    """Row b of a fresh engine that decodes the WHOLE batch with clip b's language set explicitly: one engine per
    distinct language, the batch unchanged (so the sampler's clip indices are the automatic call's)."""
    call = call or (lambda e: e.encdec_tokens_full(mel))
    out = {}
    for L in sorted(set(int(x) for x in langs)):
        e = new_engine(pkg, fix, language=L, **opts)
        ids, n = call(e)
        extra = (e.last_segments() if opts.get("timestamps") else None,
                 e.last_token_logprobs(ids.shape[1]) if opts.get("scores") else None)
        e.close()
        out[L] = (ids, n) + extra
    return out


MODES = {
    "plain": {},
    "timestamps": {"timestamps": 1},
    "scores": {"scores": 1},
    "sampling": {"temperature": 500, "seed": 1234},
    "suppress": {"suppress_default": 1},
}


@pytest.fixture(scope="module")
def detected(pkg, fix_a, mel):
    e = pkg.Engine(fix_a[0], fix_a[1], True)
    out = e.detect_language(mel)
    e.close()
    return out


def test_detection_is_the_detect_call_and_the_oracle(pkg, fix_a, mel, ref, detected):
    e = new_engine(pkg, fix_a)
    assert e.get_option("full_language") == 1
    ids, n = e.encdec_tokens_full(mel)
    lang, prob = e.last_languages()
    e.close()
    assert list(lang) == LANGS and np.array_equal(lang, detected[0])
    for i in range(len(CLIPS)):
        want = lm.softmax64(ref["z"][i])
        assert abs(float(prob[i]) - want[LANGS[i]]) <= P_TOL
        assert abs(float(prob[i]) - float(detected[1][i, LANGS[i]])) <= P_TOL
    assert np.array_equal(ids[:, 1], lm.LANG_LO + lang.astype(np.int64))
    assert np.all(ids[:, 0] == lm.SOT) and np.all(ids[:, 2] == lm.TRANSCRIBE) and np.all(ids[:, 3] == lm.NOTIMESTAMPS)
    for i in range(len(CLIPS)):
        assert [int(t) for t in ids[i, : n[i]]] == ref["rows"][(i, lm.TRANSCRIBE, P)]


@pytest.mark.parametrize("mode", list(MODES))
def test_automatic_equals_explicit(pkg, fix_a, mel, ref, mode):
    opts = MODES[mode]
    e = new_engine(pkg, fix_a, **opts)
    ids, n = e.encdec_tokens_full(mel)
    lang, _ = e.last_languages()
    segs = e.last_segments() if opts.get("timestamps") else None
    lps = e.last_token_logprobs(ids.shape[1]) if opts.get("scores") else None
    e.close()
    assert list(lang) == LANGS
    want = explicit_rows(pkg, fix_a, mel, lang, **opts)
    for i in range(len(CLIPS)):
        w = want[LANGS[i]]
        assert np.array_equal(ids[i], w[0][i]) and n[i] == w[1][i], (mode, i)
        if segs is not None:
            assert np.array_equal(segs[segs["clip"] == i], w[2][w[2]["clip"] == i])
        if mode in ("plain", "scores"):  # the oracle's greedy rows; no step of fixture A is indecisive
            assert [int(t) for t in ids[i, : n[i]]] == ref["rows"][(i, lm.TRANSCRIBE, P)]
    if lps is not None:
        en = explicit_rows(pkg, fix_a, mel, [0], **opts)[0]
        for i in range(len(CLIPS)):
            got = lps[i, 4: n[i]].astype(np.float64)
            err = float(np.abs(got - ref["lp"][i][: got.size]).max())
            print(f"clip {CLIPS[i]}: max |lp - oracle lp| = {err:.3e}; first lp {got[0]:.4f}, behind <|en|> {en[3][i, 4]:.4f}")
            assert err <= TOKEN_BOUND
            assert np.array_equal(lps[i], want[LANGS[i]][3][i])
            # the placeholder check: a chain that embedded <|en|> at position 1 would give the <|en|> value (half the 0.2
            # that tests/test_full_language_reference.py pins)
            assert abs(got[0] - float(en[3][i, 4])) > 0.1


def test_fixture_b_text_follows_the_detected_language(pkg, fix_b):
    mel8 = np.ascontiguousarray(lm.lang_mels()[list(flm.CLIPS8)])
    e = new_engine(pkg, fix_b)
    ids, n = e.encdec_tokens_full(mel8)
    lang, _ = e.last_languages()
    e.close()
    assert list(lang) == [flm.B_LANG] * 8
    own = explicit_rows(pkg, fix_b, mel8, [flm.B_LANG])[flm.B_LANG]
    en = explicit_rows(pkg, fix_b, mel8, [0])[0]
    assert np.array_equal(ids, own[0]) and np.array_equal(n, own[1])
    for i in range(8):
        assert not np.array_equal(ids[i, 4:], en[0][i, 4:]), i


CONTEXTS = [[11, 12, 13, 14, 15, 16, 17], [], [21, 22], [31, 32, 33, 34, 35]]


@pytest.mark.parametrize("kind", ["context", "ragged"])
@pytest.mark.parametrize("mode", ["plain", "scores"])
def test_behind_a_context(pkg, fix_a, mel, kind, mode):
    opts = MODES[mode]

    def call(e):
        if kind == "context":
            e.set_context(CONTEXTS[0])
        else:
            e.set_contexts(CONTEXTS)  # one empty range among them
        return e.encdec_tokens_full(mel)

    e = new_engine(pkg, fix_a, **opts)
    ids, n = call(e)
    lang, prob = e.last_languages()
    e.set_context([])
    e.set_contexts([])
    plain = e.encdec_tokens_full(mel)
    lang0, prob0 = e.last_languages()
    e.close()
    assert list(lang) == LANGS and np.array_equal(lang, lang0)  # the language of the same clip without a context
    assert np.abs(prob - prob0).max() <= 1e-6
    want = explicit_rows(pkg, fix_a, mel, lang, call=call, **opts)
    for i in range(len(CLIPS)):
        w = want[LANGS[i]]
        assert np.array_equal(ids[i], w[0][i]) and n[i] == w[1][i], (kind, i)
        n_ctx = len(CONTEXTS[0]) if kind == "context" else len(CONTEXTS[i])
        sot = n_ctx + 1 if n_ctx else 0
        assert ids[i, sot] == lm.SOT and ids[i, sot + 1] == lm.LANG_LO + LANGS[i]
    assert not np.array_equal(ids[:, : 8], plain[0][:, : 8])


def test_graphs_eager_and_replay_on_other_audio(pkg, fix_a, mel):
    other = np.ascontiguousarray(lm.lang_mels()[[22, 0, 31, 26]])  # the same shape, other languages per row
    e = new_engine(pkg, fix_a)
    a = e.encdec_tokens_full(mel)     # eager, then captured
    b = e.encdec_tokens_full(mel)     # replayed
    c = e.encdec_tokens_full(other)   # replayed on other audio: that audio's languages
    lang_c, _ = e.last_languages()
    e.set_option("use_graphs", 0)
    d = e.encdec_tokens_full(mel)
    lang_d, _ = e.last_languages()
    e.close()
    assert list(lang_c) == [94, 87, 87, 94] and list(lang_d) == LANGS
    for x in (b, d):
        assert np.array_equal(x[0], a[0]) and np.array_equal(x[1], a[1])
    assert np.array_equal(c[0][1], a[0][0]) and np.array_equal(c[0][0], a[0][1])  # clip 0 and clip 22, wherever they sit
    assert np.array_equal(c[0][2], a[0][3]) and np.array_equal(c[0][3], a[0][2])


# ------------------------------------------------------------- beam search, best_of, fall-back, word timestamps ---

# (logprob_threshold 0: no attempt is ever accepted, so the fall-back runs its whole schedule and every attempt above
# temperature 0 decodes best_of samples per clip)
WIDE = {
    "beam2": {"beam_size": 2, "full_beam": 1},
    "beam5_ts_scores": {"beam_size": 5, "full_beam": 1, "timestamps": 1, "scores": 1},
    "fallback_best_of3": {"scores": 1, "temperature_fallback": 1, "best_of": 3, "seed": 7, "logprob_threshold": 0,
                          "compression_ratio_threshold": 0},
    "beam5_in_the_fallback": {"beam_size": 5, "full_beam": 1, "fallback_beam": 1, "scores": 1, "temperature_fallback": 1,
                              "best_of": 3, "seed": 7, "logprob_threshold": 0, "compression_ratio_threshold": 0},
}


@pytest.mark.parametrize("mode", list(WIDE))
def test_beam_and_best_of_carry_each_clips_language(pkg, fix_a, mel, detected, mode):
    opts = WIDE[mode]
    if "best_of" in opts:
        opts = dict(opts, cross_absorb=1)
    e = new_engine(pkg, fix_a, **opts)
    ids, n = e.encdec_tokens_full(mel)
    lang, prob = e.last_languages()
    info = e.last_decode_info() if "temperature_fallback" in opts else None
    e.close()
    assert list(lang) == LANGS and np.array_equal(lang, detected[0])  # detection runs per clip, not per hypothesis
    assert np.abs(prob - detected[1][np.arange(4), lang]).max() <= 1e-6
    assert np.array_equal(ids[:, 1], lm.LANG_LO + lang.astype(np.int64))
    want = explicit_rows(pkg, fix_a, mel, lang, **opts)
    for i in range(len(CLIPS)):
        w = want[LANGS[i]]
        assert np.array_equal(ids[i], w[0][i]) and n[i] == w[1][i], (mode, i)
    if info is not None:
        print(mode, "attempts per clip:", info["attempts"].tolist())
        assert info["attempts"].min() > 1  # the attempts with best_of rows ran


@pytest.fixture(scope="module")
def word_vocab(fix_a, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("flang") / "word_vocab.bin")
    flm.write_word_vocab(fix_a[1], p)
    return p


def test_word_timestamps_follow_each_clips_language(pkg, fix_a, word_vocab, mel):
    """On a vocabulary of word pieces (full_language_model.WORD_PIECES) the space rule and the unicode_only rule cut the
    same ids into different words.  With the candidates {zh} every clip is Chinese and its words are those of
    wt_vocab_split_words(unicode_only = 1), with {en} those of the space rule (before the option the alignment pass took
    "en" for language = -1), and each equals, times and probabilities included, the words of a fresh engine with that
    language set explicitly: the teacher-forced rows carry the clip's own language token."""
    fix = (fix_a[0], word_vocab)
    vocab = pkg.Vocab(word_vocab, True)
    eot = lm.EOT
    found, fed = {}, {}
    for code in ("zh", "en"):
        L = pkg.language_id(code)
        e = new_engine(pkg, fix, timestamps=1, scores=1, word_timestamps=1)
        e.set_language_candidates([L])
        e.dbg_set_alignment(keep=1)
        ids, n = e.encdec_tokens_full(mel)
        fed[code] = [e.dbg_last_alignment(i) for i in range(4)]
        for al in fed[code]:  # the teacher-forced row itself: [sot, the clip's language, transcribe, notimestamps, text ..]
            assert al["row"][0] == lm.SOT and al["row"][1] == lm.LANG_LO + L and al["row"][2] == lm.TRANSCRIBE
        lang, _ = e.last_languages()
        assert list(lang) == [L] * 4 and np.all(ids[:, 1] == lm.LANG_LO + L)
        words, texts = e.last_words(with_text=True)
        segs = e.last_segments()
        e.close()
        x = new_engine(pkg, fix, language=L, timestamps=1, scores=1, word_timestamps=1)
        ids_x, n_x = x.encdec_tokens_full(mel)
        words_x, texts_x = x.last_words(with_text=True)
        x.close()
        assert np.array_equal(ids, ids_x) and np.array_equal(n, n_x)
        assert words.tobytes() == words_x.tobytes() and texts == texts_x  # every field: t0_ms, t1_ms, probability
        counts = []
        for i in range(4):
            at = [k for sg in segs[segs["clip"] == i] for k in range(sg["id_begin"], sg["id_begin"] + sg["id_count"]) if ids[i, k] < eot]
            text = [int(ids[i, k]) for k in at]
            lens = [int(v) for v in vocab.split_words(text + [eot], code == "zh")]
            kept, covered = [], 0
            for ln in lens:  # the final EOT is the last end time, not a word
                ln = min(ln, len(text) - covered)
                if ln > 0:
                    kept.append(ln)
                covered += ln
            merged = [int(v) for v in vocab.merge_punctuation(text, kept)]
            want = [at[k] for k in np.cumsum([0] + merged[:-1])] if merged else []
            mine = words[words["clip"] == i]
            assert mine["id_begin"].tolist() == want, (code, i)
            counts.append(len(want))
        found[code] = counts
    vocab.close()
    for i in range(4):  # the same text behind another language token: other attention weights of the alignment heads
        assert np.array_equal(fed["zh"][i]["row"][2:], fed["en"][i]["row"][2:])
        assert not np.array_equal(fed["zh"][i]["W"], fed["en"][i]["W"]), i
    print("words per clip: zh", found["zh"], "en", found["en"])
    # the rules differ on every clip: no piece starts with a space, so the space rule leaves one word per segment run
    assert all(z > n_en > 0 for z, n_en in zip(found["zh"], found["en"]))


# ------------------------------------------------------------------------------------------------ long form ---

def noise_pcm(seed, amp, n):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def files(pkg, fix_a):
    """Synthetic recordings of 2.5 windows whose first windows detect different languages, and one window whose own
    detection differs from its file's: found among noise at several levels with wt_detect_language_pcm."""
    e = pkg.Engine(fix_a[0], fix_a[1], True)
    win = e.pcm_len
    pool = []
    for seed in range(6):
        for amp in (0.002, 0.02, 0.2, 1.0):
            x = noise_pcm(seed, amp, win)
            pool.append((int(e.detect_language_pcm(x)[0]), x))
    e.close()
    langs = sorted(set(l for l, _ in pool))
    print("first-window languages of the pool:", [l for l, _ in pool])
    assert len(langs) >= 2, "the fixture needs windows of two languages"
    first = {L: next(x for l, x in pool if l == L) for L in langs[:2]}
    a, b = langs[:2]
    # file 0: language a, its second window would detect b; file 1: language b throughout; file 2: language a, short
    f0 = np.concatenate([first[a], first[b], first[a][: win // 2]])
    f1 = np.concatenate([first[b], first[b][::-1].copy(), first[b][: win // 2]])
    f2 = first[a][: win // 2].copy()
    return [f0, f1, f2], [a, b, None]


def long_engine(pkg, fix, language, seek, **opts):
    # (128 positions: the context a seeking loop keeps on this model, 79 ids, and the prompt behind it fit with room to spare)
    e = new_engine(pkg, fix, language=language, positions=128, timestamps=1, scores=1, **opts)
    e.set_option("seek", seek)
    return e


# Fixture A's text does not depend on the language token, its log-probabilities do (test_full_language_reference.py).
# A file's FIRST window has no context: there the language token moves the first tokens by 0.2 .. 0.5, and the window's
# log-probabilities must differ from the run behind the other language by more than ten times the numerical bar of a
# token log-probability.  Behind a context of up to 79 ids the token's weight is small (measured 2.2e-4 on one window),
# so for later windows the single-file loops are compared bit for bit: equal to the explicit run, not equal to the other.
LP_DIFFERS = 10 * TOKEN_BOUND


def long_run(e, pcm):
    text = e.transcribe_long(pcm)
    return text, e.last_token_logprobs(129), e.last_scores()["avg_logprob"].copy()


def check_windows_against(lp, explicit_lp, other_lp, rows, exact=True):
    """rows of lp against the file's explicit-language run and its run behind the other language.  exact: the same chain
    shapes ran (a single-file loop), so the rows are equal bit for bit; else (the batched loop: other batch, ragged
    kernels) each is within TOKEN_BOUND of the oracle, so the two within twice that."""
    mine = lp[rows]
    assert mine.shape == explicit_lp.shape
    if exact:
        assert np.array_equal(mine, explicit_lp)
    else:
        assert np.abs(mine.astype(np.float64) - explicit_lp).max() <= 2 * TOKEN_BOUND
    assert np.abs(mine[0].astype(np.float64) - other_lp[0]).max() > LP_DIFFERS  # the first window: no context
    for w in range(1, mine.shape[0]):
        if exact and w < other_lp.shape[0]:  # (a seeking loop behind another language may also cut other windows)
            assert not np.array_equal(mine[w], other_lp[w]), w


@pytest.mark.parametrize("seek", [0, 1])
def test_long_audio_holds_the_files_language(pkg, fix_a, files, seek):
    pcms, want = files
    e = long_engine(pkg, fix_a, -1, seek)
    for f in (0, 1):
        text, lp, avg = long_run(e, pcms[f])
        lang, prob = e.last_languages()
        assert lang.size >= 3 and list(lang) == [want[f]] * lang.size  # every window: the file's language
        assert np.all(prob == prob[0])
        x = long_engine(pkg, fix_a, want[f], seek)
        text_x, lp_x, avg_x = long_run(x, pcms[f])
        x.close()
        o = long_engine(pkg, fix_a, want[1 - f], seek)
        _, lp_o, _ = long_run(o, pcms[f])
        o.close()
        assert text == text_x and np.array_equal(avg, avg_x)
        check_windows_against(lp, lp_x, lp_o, slice(None))
    e.close()


def test_batched_seek_holds_each_files_language(pkg, fix_a, files):
    pcms, want = files
    e = long_engine(pkg, fix_a, -1, 1)
    texts = e.transcribe_long_batch(pcms)
    lp = e.last_token_logprobs(129)
    lang, prob = e.last_languages()
    wf = e.last_window_files()
    assert lang.size == wf.size == lp.shape[0]
    first = e.detect_language_pcm(pcms[2])[0]
    want = [want[0], want[1], int(first)]
    for w in range(wf.size):
        assert lang[w] == want[wf[w]], (w, wf[w])
    e.close()
    both = sorted(set(want))
    for f in range(3):
        x = long_engine(pkg, fix_a, want[f], 1)
        text_x, lp_x, _ = long_run(x, pcms[f])
        x.close()
        o = long_engine(pkg, fix_a, both[0] if want[f] != both[0] else both[1], 1)
        _, lp_o, _ = long_run(o, pcms[f])
        o.close()
        assert texts[f] == text_x, f
        check_windows_against(lp, lp_x, lp_o, np.nonzero(wf == f)[0], exact=False)


# ------------------------------------------------------------------------------------------------ candidates ---

def test_candidates(pkg, fix_a, mel, detected):
    L = pkg.lib()
    e = new_engine(pkg, fix_a)
    base = e.encdec_tokens_full(mel)
    base_lang = e.last_languages()
    base_det = e.detect_language(mel)
    assert e.get_option("language_candidates") == 0
    e.set_language_candidates([87, 87])  # duplicates count once
    assert e.get_option("language_candidates") == 1
    lang, probs = e.detect_language(mel)
    assert list(lang) == [87] * 4 and np.all(probs[:, 87] == 1.0) and np.all(np.delete(probs, 87, axis=1) == 0.0)
    ids, n = e.encdec_tokens_full(mel)
    fl, fp = e.last_languages()
    assert list(fl) == [87] * 4 and np.all(fp == 1.0) and np.all(ids[:, 1] == lm.LANG_LO + 87)  # clip 22 is forced to 87
    want = explicit_rows(pkg, fix_a, mel, [87])[87]
    assert np.array_equal(ids, want[0]) and np.array_equal(n, want[1])
    e.set_language_candidates([94, 87])
    assert e.get_option("language_candidates") == 2
    lang, probs = e.detect_language(mel)
    assert list(lang) == LANGS
    for i in range(4):
        p2 = detected[1][i].astype(np.float64)[[87, 94]]
        p2 /= p2.sum()
        assert np.abs(probs[i, [87, 94]] - p2).max() <= P_TOL and probs[i].sum() == pytest.approx(1.0, abs=1e-5)
        assert np.all(np.delete(probs[i], [87, 94]) == 0.0)
    ids2, n2 = e.encdec_tokens_full(mel)
    fl2, fp2 = e.last_languages()
    assert list(fl2) == LANGS and np.array_equal(ids2, base[0])
    assert np.abs(fp2 - probs[np.arange(4), fl2]).max() <= 1e-6
    # the 31-position automatic decode, synchronous and in the pipeline (its own graphs: the key's language mode + 2)
    e.set_option("max_positions", 0)
    e.set_language_candidates([87])
    ids31, n31 = e.encdec_tokens_batch(mel)
    assert np.all(ids31[:, 1] == lm.LANG_LO + 87) and list(e.last_languages()[0]) == [87] * 4
    dev = e.device_array(mel)
    for _ in range(2):  # eager and captured, then replayed
        e.pipeline_submit_dev(dev.data_ptr(), 4)
        ids_p, n_p = e.pipeline_collect()
        assert np.array_equal(ids_p, ids31) and np.array_equal(n_p, n31)
    e.set_language_candidates([94, 87])
    e.pipeline_submit_dev(dev.data_ptr(), 4)  # the mask is device data: the same graphs, the other list
    ids_p, n_p = e.pipeline_collect()
    assert list(ids_p[:, 1] - lm.LANG_LO) == LANGS
    dev.free()
    e.set_language_candidates([87])
    e.set_language_candidates([])
    auto31 = e.encdec_tokens_batch(mel)
    assert list(auto31[0][:, 1] - lm.LANG_LO) == LANGS
    e.set_option("max_positions", P)
    # cleared: the earlier outputs bit for bit
    again = e.encdec_tokens_full(mel)
    again_lang = e.last_languages()
    again_det = e.detect_language(mel)
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1])
    assert np.array_equal(again_lang[0], base_lang[0]) and again_lang[1].tobytes() == base_lang[1].tobytes()
    assert again_det[1].tobytes() == base_det[1].tobytes()
    for bad in ([-1], [99], [0] * 129):
        with pytest.raises(pkg.WtError) as x:
            e.set_language_candidates(bad)
        assert status_of(x) == INVALID
    assert e.get_option("language_candidates") == 0
    with pytest.raises(pkg.WtError) as x:
        e.set_option("language_candidates", 1)
    assert status_of(x) == INVALID
    e.close()
    for eng in (pkg.Engine(fix_a[0], fix_a[1], True, pkg.EngineType.Monolith), pkg.Engine(fix_a[0], fix_a[1], False)):
        with pytest.raises(pkg.WtError) as x:
            eng.set_language_candidates([1])
        assert status_of(x) == UNSUPPORTED
        eng.close()
    assert L.wt_engine_set_language_candidates(None, None, 0) == 1


# ------------------------------------------------------------------------------------------------------ task ---

def test_task_translate(pkg, assets, fix_a, mel, ref):
    e = new_engine(pkg, fix_a)
    assert e.get_option("task") == 0
    e.set_option("task", 1)
    ids, n = e.encdec_tokens_full(mel)
    for i in range(4):
        assert [int(t) for t in ids[i, : n[i]]] == ref["rows"][(i, flm.TRANSLATE, P)]
    e.set_option("max_positions", 0)
    ids31, n31 = e.encdec_tokens_batch(mel)  # the 31-position automatic call
    for i in range(4):
        assert [int(t) for t in ids31[i, : n31[i]]] == ref["rows"][(i, flm.TRANSLATE, 30)]
    e.set_prompt(flm.prompt_for(2))
    with pytest.raises(pkg.WtError) as x:
        e.encdec_tokens_batch(mel)
    assert status_of(x) == UNSUPPORTED and "task" in str(x.value)
    e.set_prompt([])
    for bad in (-1, 2):
        with pytest.raises(pkg.WtError) as x:
            e.set_option("task", bad)
        assert status_of(x) == INVALID
    e.set_option("task", 0)
    back = e.encdec_tokens_batch(mel)
    assert np.all(back[0][:, 2] == lm.TRANSCRIBE)
    e.close()
    prefix, vocab = assets("micro")
    for eng in (pkg.Engine(fix_a[0], fix_a[1], True, pkg.EngineType.Monolith), pkg.Engine(fix_a[0], fix_a[1], False),
                pkg.Engine(prefix, vocab, True)):  # Monolith, English-only, a vocabulary that ends before <|translate|>
        with pytest.raises(pkg.WtError) as x:
            eng.set_option("task", 1)
        assert status_of(x) == UNSUPPORTED
        assert eng.get_option("task") == 0
        eng.close()


# ------------------------------------------------------------------------------------- refusals and defaults ---

def test_refusals_and_unchanged_defaults(pkg, fix_a, mel):
    import ctypes
    L = pkg.lib()
    e = pkg.Engine(fix_a[0], fix_a[1], True)
    e.set_option("max_positions", P)
    assert e.get_option("full_language") == 0
    explicit = e.encdec_tokens_full(mel)  # language 2
    e.set_option("language", -1)

    def refused(fn, word="language"):
        with pytest.raises(pkg.WtError) as x:
            fn()
        assert status_of(x) == UNSUPPORTED and word in str(x.value), str(x.value)

    refused(lambda: e.encdec_tokens_full(mel))  # full_language = 0: the refusal stands
    for bad in (-1, 2):
        with pytest.raises(pkg.WtError) as x:
            e.set_option("full_language", bad)
        assert status_of(x) == INVALID
    e.set_option("full_language", 1)
    want = e.encdec_tokens_full(mel)
    e.set_prompt(flm.prompt_for(2))
    refused(lambda: e.encdec_tokens_full(mel), "prompt")
    e.set_prompt([])
    forced = np.zeros((4, 32), np.int64)
    forced[:, :4] = lm.prompt_for(2)
    assert L.wt_dbg_set_forced_ids(e.handle, forced.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 4) == 0
    refused(lambda: e.encdec_tokens_full(mel), "forced")
    assert L.wt_dbg_set_forced_ids(e.handle, None, 0) == 0
    e.set_option("bf16", 1)
    refused(lambda: e.encdec_tokens_full(mel), "bf16")
    e.set_option("bf16", 0)
    dev = e.device_array(mel)
    refused(lambda: e.pipeline_submit_dev(dev.data_ptr(), 4), "pipeline")
    e._submitted = []
    dev.free()
    # the 31-position beam stays refused, and a full-length beam without full_beam as ever
    e.set_option("beam_size", 2)
    refused(lambda: e.encdec_tokens_full(mel), "beam")
    e.set_option("max_positions", 0)
    refused(lambda: e.encdec_tokens_batch(mel), "beam")
    e.set_option("max_positions", P)
    e.set_option("beam_size", 1)
    again = e.encdec_tokens_full(mel)  # the engine is usable and gives the same result
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    e.set_option("full_language", 0)
    e.set_option("language", 2)
    back = e.encdec_tokens_full(mel)
    assert np.array_equal(back[0], explicit[0]) and np.array_equal(back[1], explicit[1])
    with pytest.raises(pkg.WtError):
        e.last_languages()  # an explicit call reports none
    e.close()
    mono = pkg.Engine(fix_a[0], fix_a[1], True, pkg.EngineType.Monolith)
    refused(lambda: mono.set_option("language", -1))
    mono.close()
