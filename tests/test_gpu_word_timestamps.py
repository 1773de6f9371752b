"""GPU (-m gpu): word-level timestamps end to end (option word_timestamps) on the timestamp model
of tests/ts_model.py.  Two levels: the continuous stages the engine formed (attention weights W, cost C) are held to the
float64 restatement of tests/align_ref.py over the engine's own encoder output and id row; the discrete stages are exact
on identical input: jump = align_ref.dtw of the engine's own C, words = align_ref.words of that jump."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import align_ref  # noqa: E402
import ts_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
# The weights against float64, relative, at the bar of tests/test_gpu_align_kernels.py.  Here the queries come out of the
# engine's own decoder layers (fp32-level GEMMs) and the reference's out of float64 ones: measured
# 3.9e-6.  The cost, scaled by max(1, |C|), inherits that error through (W - mean) / std, where it grows by mean / std:
# measured 2.7e-6 (the stage kernels alone, on identical W: 9.5e-8); the bar is a decade above.
W_BOUND, C_BOUND = 1e-4, 3e-5
NOT = 50363  # <|notimestamps|> of the multilingual vocabulary


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def model(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("words") / "micro-ts")
    tm.write_model(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def weights(model):
    from wtw import read_wtw
    return read_wtw(model[0] + ".wtw")


@pytest.fixture(scope="module")
def mel():
    m = tm.mels(32)
    m.setflags(write=False)
    return m


@pytest.fixture(scope="module")
def eng(pkg, model):
    e = pkg.Engine(model[0], model[1], True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def enc_out(eng, mel):
    """The engine's own encoder output, from a plain call before any option is set."""
    eng.set_prompt([3, 5, 7, 11])
    _, _, enc, _ = eng.encdec_debug_batch(mel, want_logits=False)
    eng.set_prompt([])
    return enc


def decode(eng, mel, positions, scores=1, heads=(), mode=1, sub=0):
    eng.set_option("max_positions", positions)
    eng.set_option("timestamps", 1)
    eng.set_option("scores", scores)
    eng.set_option("word_timestamps", 1)
    eng.dbg_set_alignment(keep=1, mode=mode, sub=sub)
    eng.set_alignment_heads(heads)
    try:
        return eng.encdec_tokens_full(mel)
    finally:
        eng.dbg_set_alignment(keep=0, mode=1, sub=0)
        for k in ("word_timestamps", "scores", "timestamps", "max_positions"):
            eng.set_option(k, 0)


def check_clips(pkg, eng, model, weights, enc, ids, n, positions, heads=None, frames=None):
    dims, tensors = weights
    vocab = pkg.Vocab(model[1], True)
    segs = eng.last_segments()
    words, texts = eng.last_words(with_text=True)
    try:
        lp = eng.last_token_logprobs(positions + 1)
    except pkg.WtError:
        lp = None
    heads = sorted(heads or align_ref.default_heads(dims))
    worst_w = worst_c = 0.0
    at_word = moved = boundaries = 0
    for b in range(ids.shape[0]):
        al = eng.dbg_last_alignment(b)
        row = [int(i) for i in ids[b, :n[b]]]
        # the text: the ids below EOT inside the clip's segments
        where = [k for s in segs[segs["clip"] == b] for k in range(s["id_begin"], s["id_begin"] + s["id_count"]) if row[k] < tm.EOT]
        text = [row[k] for k in where]
        n_a = len(tm.PROMPT)
        cap = dims["n_text_ctx"] - n_a - 2
        text, where = text[:cap], where[:cap]
        F = dims["n_audio_ctx"] if frames is None else frames[b]
        assert list(al["row"]) == tm.PROMPT + [NOT] + text + [tm.EOT]
        assert (al["n_a"], al["L"], al["N"], al["F"], al["heads"]) == (n_a, n_a + len(text) + 2, len(text) + 1, F, len(heads))
        W64 = align_ref.weights(dims, tensors, list(al["row"]), enc[b], heads, F)
        big = W64 > 1e-30
        worst_w = max(worst_w, float((np.abs(al["W"] - W64)[big] / W64[big]).max()))
        assert np.all(al["W"][:, :, F:] == 0)
        C64 = align_ref.cost_matrix(W64, al["L"], F, n_a)
        worst_c = max(worst_c, float(np.abs(al["C"][:, :F] - C64).max() / max(1.0, np.abs(C64).max())))
        # the discrete stages on the engine's own C
        jump = align_ref.dtw(al["C"][:, :F])[0]
        assert np.array_equal(al["jump"], jump), b
        mine = words[words["clip"] == b]
        if not text:
            assert mine.size == 0
            continue
        toks = [vocab.token(i) for i in text + [tm.EOT]]
        want = align_ref.words(toks, text + [tm.EOT], tm.EOT, jump)
        assert mine.size == len(want), (b, mine, want)
        # information, no bar: the word boundaries that move when DTW runs on the float64 cost instead
        want64 = align_ref.words(toks, text + [tm.EOT], tm.EOT, align_ref.dtw(C64)[0])
        boundaries += 2 * len(want)
        moved += sum((a[2] != c[2]) + (a[3] != c[3]) for a, c in zip(want, want64))
        for w, (s0, cnt, t0, t1) in zip(mine, want):
            assert (w["t0_ms"], w["t1_ms"]) == (t0, t1)
            assert (w["id_begin"], w["id_count"]) == (where[s0], where[s0 + cnt - 1] - where[s0] + 1)
            seg = segs[w["segment"]]
            assert seg["clip"] == b and seg["id_begin"] <= w["id_begin"] < seg["id_begin"] + seg["id_count"]
            assert texts[at_word] == b"".join(toks[s0:s0 + cnt])
            if lp is None:
                assert w["probability"] == 0
            else:  # the mean of exp(log-probability): the engine's own fp32 values, one exp and a mean away
                p = float(np.mean(np.exp(lp[b, [where[s0 + k] for k in range(cnt)]].astype(np.float64))))
                assert abs(w["probability"] - p) <= 1e-6
            at_word += 1
    assert at_word == words.size
    vocab.close()
    print(f"word timestamps clips={ids.shape[0]} P={positions} heads={len(heads)}: W rel err {worst_w:.3g}, C err {worst_c:.3g}, "
          f"{words.size} words, {moved} of {boundaries} word boundaries differ under a float64 DTW")
    assert worst_w <= W_BOUND and worst_c <= C_BOUND


@pytest.mark.parametrize("positions,batch", [(tm.P_SHORT, 1), (tm.P_LONG, 5), (tm.P_LONG, 32), (tm.P_SHORT, 32)])
def test_alignment_and_words(pkg, eng, model, weights, mel, enc_out, positions, batch):
    """Batches 1 and 5 decode on the cached cross-attention, 32 on the absorbed one; the alignment pass is the same."""
    ids, n = decode(eng, mel[:batch], positions)
    check_clips(pkg, eng, model, weights, enc_out[:batch], ids, n, positions)


@pytest.mark.parametrize("mode,sub", [(0, 0), (1, 3), (0, 7)])
def test_other_forms_of_the_pass(pkg, eng, model, weights, mel, enc_out, mode, sub):
    """The fused form of align_scores, and sub-groups of 3 and 7 clips (the last one shorter) in place of one of 32."""
    ids, n = decode(eng, mel, tm.P_LONG, mode=mode, sub=sub)
    check_clips(pkg, eng, model, weights, enc_out, ids, n, tm.P_LONG)


def test_custom_heads_and_no_scores(pkg, eng, model, weights, mel, enc_out):
    heads = [(1, 0), (0, 1)]
    ids, n = decode(eng, mel[:5], tm.P_LONG, scores=0, heads=heads)
    assert eng.get_option("alignment_heads") == 2
    custom = eng.dbg_last_alignment(0)["W"]
    check_clips(pkg, eng, model, weights, enc_out[:5], ids, n, tm.P_LONG, heads=heads)
    ids, n = decode(eng, mel[:5], tm.P_LONG, scores=0)
    default = eng.dbg_last_alignment(0)["W"]
    assert eng.get_option("alignment_heads") == default.shape[0] == 2  # the default: both heads of layer 1
    # sorted by (layer, head): custom = (0, 1), (1, 0); default = (1, 0), (1, 1)
    assert not np.array_equal(custom[0], default[0]) and np.array_equal(custom[1].view(np.uint32), default[0].view(np.uint32))


def test_refusals_leave_the_engine_usable(pkg, eng, mel, model, weights, enc_out):
    eng.set_option("word_timestamps", 1)
    try:
        with pytest.raises(pkg.WtError) as err:  # neither timestamps nor max_positions
            eng.encdec_tokens_batch(mel[:1])
        assert status_of(err) == UNSUPPORTED
        eng.set_option("max_positions", tm.P_SHORT)
        with pytest.raises(pkg.WtError) as err:  # no timestamps
            eng.encdec_tokens_full(mel[:1])
        assert status_of(err) == UNSUPPORTED
        eng.set_option("timestamps", 1)
        eng.set_option("cross_absorb", 0)
        with pytest.raises(pkg.WtError) as err:  # no absorbed form
            eng.encdec_tokens_full(mel[:1])
        assert status_of(err) == UNSUPPORTED
        eng.set_option("cross_absorb", 1)
    finally:
        for k in ("word_timestamps", "timestamps", "max_positions"):
            eng.set_option(k, 0)
    for bad in ([(4, 0)], [(0, 2)], [(0, 0), (0, 0)], [(0, 0)] * 129):
        with pytest.raises(pkg.WtError) as err:
            eng.set_alignment_heads(bad)
        assert status_of(err) == INVALID
    eng.set_option("max_positions", tm.P_SHORT)
    eng.set_option("timestamps", 1)
    eng.encdec_tokens_full(mel[:1])
    with pytest.raises(pkg.WtError):  # that decode ran without the option
        eng.last_words()
    eng.set_option("timestamps", 0)
    eng.set_option("max_positions", 0)
    ids, n = decode(eng, mel[:1], tm.P_SHORT)
    check_clips(pkg, eng, model, weights, enc_out[:1], ids, n, tm.P_SHORT)


def pcm_clip(seed, n):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.3 * np.sin(2 * np.pi * (220 + 40 * seed) * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)


def test_frames_follow_the_pcm_length(pkg, eng, model, weights):
    """A clip that comes in as PCM is aligned over the frames of its own samples: floor(samples / 320), at least 1 and at
    most n_audio_ctx (this model's window is 32 000 samples, 100 frames).  The words' times stay inside them."""
    win = 160 * eng.mel_shape[1]
    for n_samples, frames in ((13123, 41), (win, 100), (win + 5000, 100), (100, 1)):
        for k, v in (("max_positions", tm.P_SHORT), ("timestamps", 1), ("word_timestamps", 1)):
            eng.set_option(k, v)
        eng.dbg_set_alignment(keep=1)
        try:
            eng.transcribe(pcm_clip(1, n_samples))
            al = eng.dbg_last_alignment(0)
            words = eng.last_words()
        finally:
            eng.dbg_set_alignment(keep=0)
            for k in ("word_timestamps", "timestamps", "max_positions"):
                eng.set_option(k, 0)
        assert al["F"] == frames and np.all(al["W"][:, :, frames:] == 0)
        assert np.array_equal(al["jump"], align_ref.dtw(al["C"][:, :frames])[0])
        assert words.size > 0 and words["t1_ms"].max() <= 20 * (frames - 1) and np.all(words["t0_ms"] <= words["t1_ms"])
        assert np.all(np.diff(words["t0_ms"]) >= 0)


def check_windows(pkg, eng, model, n_windows, offset_ms, frames):
    """After a transcribe_long: per window the discrete stages on what the engine itself formed (the float64 forward
    needs a window's encoder output, which a long call does not hand out: the single-call tests hold W to it).  C equals
    the float64 cost of the engine's own W at the stage kernels' bar, jump = align_ref.dtw of the engine's own C, and the
    words of the window are align_ref.words of that jump over the text the row holds, offset_ms(w) later."""
    vocab = pkg.Vocab(model[1], True)
    words, texts = eng.last_words(with_text=True)
    segs = eng.last_segments()
    assert sorted(set(words["clip"].tolist())) == [w for w in range(n_windows) if eng.dbg_last_alignment(w)["L"] > len(tm.PROMPT) + 2]
    at = 0
    for w in range(n_windows):
        al = eng.dbg_last_alignment(w)
        mine = words[words["clip"] == w]
        if al["L"] <= len(tm.PROMPT) + 2:  # nothing kept from the window
            assert mine.size == 0
            continue
        n_a, F = al["n_a"], al["F"]
        assert F == frames[w] and list(al["row"][:n_a + 1]) == tm.PROMPT + [NOT] and al["row"][-1] == tm.EOT
        text = [int(i) for i in al["row"][n_a + 1:-1]]
        assert all(i < tm.EOT for i in text)
        C64 = align_ref.cost_matrix(al["W"], al["L"], F, n_a)
        assert np.abs(al["C"][:, :F] - C64).max() / max(1.0, np.abs(C64).max()) <= 1e-6
        jump = align_ref.dtw(al["C"][:, :F])[0]
        assert np.array_equal(al["jump"], jump)
        toks = [vocab.token(i) for i in text + [tm.EOT]]
        want = align_ref.words(toks, text + [tm.EOT], tm.EOT, jump)
        assert mine.size == len(want)
        for wd, (s0, cnt, t0, t1) in zip(mine, want):
            assert (wd["t0_ms"], wd["t1_ms"]) == (t0 + offset_ms(w), t1 + offset_ms(w))
            assert texts[at] == b"".join(toks[s0:s0 + cnt])
            sg = segs[wd["segment"]]
            assert sg["clip"] == w and sg["id_begin"] <= wd["id_begin"] and wd["id_begin"] + wd["id_count"] <= sg["id_begin"] + sg["id_count"]
            assert wd["id_count"] >= cnt
            at += 1
    assert at == words.size
    vocab.close()
    return words


def long_call(eng, pcm, seek):
    for k, v in (("max_positions", tm.P_SHORT), ("timestamps", 1), ("word_timestamps", 1), ("seek", seek)):
        eng.set_option(k, v)
    eng.dbg_set_alignment(keep=1)
    try:
        eng.transcribe_long(pcm)
    finally:
        eng.dbg_set_alignment(keep=0)
        for k in ("seek", "word_timestamps", "timestamps", "max_positions"):
            eng.set_option(k, 0)


def test_long_audio_numbers_the_windows(pkg, eng, model):
    """wt_transcribe_long_pcm in fixed windows: clip = the window's index, the times are the file's (30 000 ms per
    window, as the segments'), a word's segment index counts through the whole file; the last window is short."""
    win = 160 * eng.mel_shape[1]
    long_call(eng, pcm_clip(2, 2 * win + win // 2), 0)
    words = check_windows(pkg, eng, model, 3, lambda w: 30000 * w, [100, 100, 50])
    assert sorted(set(words["clip"].tolist())) == [0, 1, 2]


def test_seeking_long_audio(pkg, eng, model):
    """seek = 1: every window is aligned over the segments seek_step kept of it (a word may span a timestamp id), clip =
    the window, the times start at seek_sample / 16 ms, the frames are those of the samples the window holds."""
    win = 160 * eng.mel_shape[1]
    pcm = pcm_clip(3, 3 * win + 4321)
    long_call(eng, pcm, 1)
    wins = eng.last_windows()
    assert len(wins) >= 3
    frames = [min(100, max(1, min(win, pcm.size - int(w["seek_sample"])) // 320)) for w in wins]
    words = check_windows(pkg, eng, model, len(wins), lambda w: int(wins[w]["seek_sample"]) // 16, frames)
    assert words.size > 0 and len(set(words["clip"].tolist())) >= 2


def test_text_beyond_the_cap_forms_no_words(pkg, assets, tmp_path, mel):
    """L > full_cap(): with a quiet EOT row and timestamp rows that are not amplified, a decode over all 128 positions
    yields one opening timestamp and 125 text ids; the alignment row has room for 128 - 3 - 2 = 123 of them, the first 123
    are aligned and the others form no words."""
    prefix, vocab = assets("micro")
    p = str(tmp_path / "micro-long")
    tm.write_model(prefix + ".wtw", p + ".wtw", ts_gain=1.0, rich=(0.5, tm.RICH[1], tm.RICH[2]))
    from wtw import read_wtw
    e = pkg.Engine(p, vocab, True)
    clips = mel[:5]
    try:
        e.set_prompt([3, 5, 7, 11])
        _, _, enc, _ = e.encdec_debug_batch(clips, want_logits=False)
        e.set_prompt([])
        ids, n = decode(e, clips, tm.N_TEXT_CTX)
        segs = e.last_segments()
        n_text = [sum(1 for s in segs[segs["clip"] == b] for k in range(s["id_begin"], s["id_begin"] + s["id_count"]) if ids[b, k] < tm.EOT)
                  for b in range(clips.shape[0])]
        print("text ids per clip:", n_text)
        assert max(n_text) > 123, "no clip of this model overflows the alignment row: the case is not exercised"
        for b in range(clips.shape[0]):
            assert e.dbg_last_alignment(b)["L"] == 3 + 1 + min(n_text[b], 123) + 1 <= tm.N_TEXT_CTX
        check_clips(pkg, e, (p, vocab), read_wtw(p + ".wtw"), enc, ids, n, tm.N_TEXT_CTX)
    finally:
        e.close()
