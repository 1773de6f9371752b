"""Which last_* getters answer, and with how many entries, after each kind of decode call on ONE engine (DESIGN.md
section 29: the engine keeps what a decode leaves behind in one record, and every entry point forgets a fixed set of
its groups).  The expected table was printed by this file run against the build of the commit before the record
existed and pasted in here; the test uses the public Python surface alone, so it passes on that build and on this one.

The model is the seeking tests' (tests/longform_model.py over the micro weights) at max_positions = 32.  With so few
positions a window's context must stay empty, so the seeking steps run with condition_on_previous_text = 0."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import DevBuf  # noqa: E402
import longform_model as lm  # noqa: E402

pytestmark = pytest.mark.gpu

P = 32
GETTERS = ("segments", "words", "scores", "token_logprobs", "decode_info", "best_of", "windows", "window_files",
           "languages", "beam_scores", "alignment")
R = "refused"
# step -> what every getter of GETTERS gave, in that order
EXPECTED = {
    "1 full: timestamps + scores + words, 2 clips": (2, 44, 2, 2, R, R, R, R, R, R, 2),
    "2 short: encdec_tokens_batch, 1 clip": (R, 44, R, R, R, R, R, R, R, R, 2),
    "3 pipeline: submit_dev + collect, 2 clips": (R, 44, R, R, R, R, R, R, R, R, 2),
    "4 transcribe_long, seek 0, 33 windows": (33, 957, 33, 33, R, R, R, R, R, R, 1),
    "5 transcribe_long, seek 1": (3, 87, 3, 3, R, R, 3, R, R, R, 3),
    "6 transcribe_long_batch, 2 files": (5, R, 5, 5, R, R, 5, 5, R, R, R),
    "7 beam: encdec_tokens_batch, 2 clips": (R, R, R, R, R, R, R, R, R, 2, R),
    "8 language auto: encdec_tokens_batch, 2 clips": (R, R, R, R, R, R, R, R, 2, R, R),
}


def state(pkg, eng):
    def size(fn):
        try:
            v = fn()
        except pkg.WtError:
            return R
        return int(len(v[0] if isinstance(v, tuple) else v))

    def alignment():  # the clips the tap answers for
        n = 0
        try:
            while True:
                eng.dbg_last_alignment(n)
                n += 1
        except pkg.WtError:
            return n if n else R

    return (size(eng.last_segments), size(eng.last_words), size(eng.last_scores), size(lambda: eng.last_token_logprobs(P + 1)),
            size(eng.last_decode_info), size(eng.last_best_of), size(eng.last_windows), size(eng.last_window_files),
            size(eng.last_languages), size(eng.last_beam_scores), alignment())


def options(eng, **kw):
    """Every option the steps touch, back to its default unless named."""
    want = dict(word_timestamps=0, seek=0, beam_size=1, language=2, scores=0, timestamps=0, max_positions=0,
                condition_on_previous_text=1)
    want.update(kw)
    for k in ("word_timestamps", "seek", "beam_size", "language", "max_positions", "timestamps", "scores",
              "condition_on_previous_text"):
        eng.set_option(k, want[k])


def test_which_getters_answer_after_each_entry_point(pkg, assets, tmp_path):
    prefix, vocab = assets("micro")
    p = str(tmp_path / "micro-longform")
    lm.write_model(prefix + ".wtw", p + ".wtw")
    eng = pkg.Engine(p, vocab, True)
    rng = np.random.default_rng(11)
    mel = rng.uniform(-1.0, 1.5, size=(2,) + eng.mel_shape).astype(np.float32)
    audio = (0.3 * rng.standard_normal(33 * lm.WIN - 3000)).astype(np.float32)
    full = dict(max_positions=P, timestamps=1, scores=1)
    got = {}
    steps = iter(EXPECTED)
    try:
        eng.dbg_set_alignment(keep=1)
        options(eng, word_timestamps=1, **full)
        eng.encdec_tokens_full(mel)
        got[next(steps)] = state(pkg, eng)

        options(eng)
        eng.encdec_tokens_batch(mel[:1])
        got[next(steps)] = state(pkg, eng)

        buf = DevBuf(mel)
        try:
            eng.pipeline_submit_dev(buf.data_ptr(), 2)
            eng.pipeline_collect()
        finally:
            buf.free()
        got[next(steps)] = state(pkg, eng)

        options(eng, word_timestamps=1, **full)
        assert len(eng.transcribe_long(audio).split("\n")) == 33  # two batches: 32 windows and 1
        got[next(steps)] = state(pkg, eng)

        options(eng, word_timestamps=1, seek=1, condition_on_previous_text=0, **full)
        eng.transcribe_long(audio[: 3 * lm.WIN - 3000])
        got[next(steps)] = state(pkg, eng)

        options(eng, condition_on_previous_text=0, **full)
        assert len(eng.transcribe_long_batch([audio[: 2 * lm.WIN - 3000], audio[lm.WIN: 4 * lm.WIN]])) == 2
        got[next(steps)] = state(pkg, eng)

        options(eng, beam_size=2)
        eng.encdec_tokens_batch(mel)
        got[next(steps)] = state(pkg, eng)

        options(eng, language=-1)
        eng.encdec_tokens_batch(mel)
        got[next(steps)] = state(pkg, eng)
    finally:
        eng.close()
    print("GETTERS =", GETTERS)
    for k, v in got.items():
        print("    %r: %r," % (k, v))
    assert got == EXPECTED
