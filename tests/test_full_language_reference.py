"""The fixtures of the full-length automatic-language tests (tests/full_language_model.py) on the CPU oracle, so that
they cannot drift.  CPU only.  This file pins oracle values that the GPU tests lean on; it does not test the feature and
passes with or without it (the tests that fail without the feature are the two GPU files).

Fixture A (the language model at 160 positions): the languages are 87 for 29 clips and 94 for clips 22, 24 and 26, the
smallest top-two language gap 0.0703 — the 31-position fixture's.  Greedy decodes of clips 0, 1, 2, 22, 24, 26 and 31
behind their own prompt run to the cap at 96 positions; the smallest step margin is 0.154 with the transcribe prompt and
0.037 with the translate prompt, far above full_model.MARGIN = 2e-4.  Text does not depend on the language token here,
so the placeholder check is on a log-probability: between the clip's own language prompt and the <|en|> prompt the first
generated token's log-probability moves by 0.228 .. 0.567 on eight clips (asserted >= 0.2).
Fixture B (A with the self-attention out weights x 4): all eight clips detect language 50 with gaps >= 3.76, all decode
differently behind <|en|> than behind 50 at 48 positions, smallest step margin 0.0055."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import full_language_model as flm  # noqa: E402
import full_model as fm  # noqa: E402
import lang_model as lm  # noqa: E402


def open_model(orc, assets, tmp_path_factory, writer, name):
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("flang") / name)
    writer(prefix + ".wtw", p + ".wtw")
    return orc.Model(p + ".wtw")


@pytest.fixture(scope="module")
def model_a(orc, assets, tmp_path_factory):
    m = open_model(orc, assets, tmp_path_factory, flm.write_a, "micro-flang-a")
    yield m
    m.close()


@pytest.fixture(scope="module")
def model_b(orc, assets, tmp_path_factory):
    m = open_model(orc, assets, tmp_path_factory, flm.write_b, "micro-flang-b")
    yield m
    m.close()


@pytest.fixture(scope="module")
def enc_a(model_a):
    mel = lm.lang_mels()
    return {b: model_a.encode(mel[b]) for b in range(lm.N_CLIPS)}


def test_fixture_a_languages_and_gaps(model_a, enc_a):
    assert model_a.dims["n_text_ctx"] == fm.N_TEXT_CTX
    langs, gaps = [], []
    for b in range(lm.N_CLIPS):
        _, lang, gap = lm.oracle_language(model_a, enc_a[b])
        langs.append(lang)
        gaps.append(gap)
    print("languages", langs, "smallest gap", min(gaps))
    assert langs == lm.EXPECT_LANGS
    assert [langs[b] for b in flm.CLIPS] == [87, 94, 94, 87]
    assert abs(min(gaps) - 0.0703) < 5e-4  # unchanged from the 31-position fixture: position 0 sees no later row


def test_fixture_a_decodes_are_decisive_under_both_tasks(model_a, enc_a):
    for task, floor in ((lm.TRANSCRIBE, 0.15), (flm.TRANSLATE, 0.035)):  # measured 0.154 and 0.037
        margins = []
        for b in (0, 1, 2, 22, 24, 26, 31):
            ids, margin, _ = flm.decode(model_a, enc_a[b], flm.prompt_for(lm.EXPECT_LANGS[b], task), 96)
            assert len(ids) == 97 and ids[-1] != lm.EOT  # to the cap
            margins.append(margin)
        print("task", task, "smallest step margin", min(margins))
        assert min(margins) > floor > 100 * fm.MARGIN


def test_fixture_a_first_logprob_tells_the_placeholder(model_a, enc_a):
    moves = []
    for b in flm.CLIPS8:
        own = flm.decode(model_a, enc_a[b], flm.prompt_for(lm.EXPECT_LANGS[b]), 48)
        en = flm.decode(model_a, enc_a[b], flm.prompt_for(0), 48)
        moves.append(abs(own[2] - en[2]))
    print("first generated token: |lp(own language) - lp(<|en|>)|", [round(m, 3) for m in moves])
    assert min(moves) >= 0.2  # measured 0.228 .. 0.567


def test_fixture_a_translate_rows_of_the_gpu_clips(model_a, enc_a):
    # the rows tests/test_gpu_full_language.py compares its task = 1 calls with: every step decisive, at 31 and 48 positions
    for b in flm.CLIPS:
        for positions in (30, 48):
            ids, margin, _ = flm.decode(model_a, enc_a[b], flm.prompt_for(lm.EXPECT_LANGS[b], flm.TRANSLATE), positions)
            assert ids[2] == flm.TRANSLATE and margin > 10 * fm.MARGIN, (b, positions, margin)


def test_fixture_b_text_depends_on_the_language(model_b):
    mel = lm.lang_mels()
    margins, gaps = [], []
    for b in flm.CLIPS8:
        enc = model_b.encode(mel[b])
        _, lang, gap = lm.oracle_language(model_b, enc)
        assert lang == flm.B_LANG
        gaps.append(gap)
        own = flm.decode(model_b, enc, flm.prompt_for(lang), 48)
        en = flm.decode(model_b, enc, flm.prompt_for(0), 48)
        assert own[0][4:] != en[0][4:], b  # all eight differ
        margins.append(own[1])
    print("fixture B: language gaps", min(gaps), "smallest step margin", min(margins))
    assert min(gaps) >= 3.7  # measured 3.76
    assert min(margins) > 10 * fm.MARGIN  # measured 0.0055
