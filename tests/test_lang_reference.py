"""The fixture of the spoken-language tests (tests/lang_model.py) on the CPU oracle, so that it cannot drift: which
languages the 32 clips have and how far apart the top two language logits are, and how decisive the greedy steps
behind the detected prompt are.  CPU only.

Measured on the oracle: language 87 for 29 clips and 94 for clips 22, 24 and 26; smallest top-two language gap 0.0703,
median 2.39; the 32 clips' greedy steps behind their own prompt have a smallest top-two margin of 0.0225.  For 8 clips
of the uniform generator of tests/test_gpu_beam.py behind their detected prompt, the first generated step has the
smallest margin, 0.1105, and every later step 18.7 or more (asserted: 0.195 for the later steps).  All of it is far above the 2e-4
decision margin of tests/test_gpu_language.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lang_model as lm  # noqa: E402

DECISION_MARGIN = 2e-4  # tests/test_gpu_language.py: twice the project's logits bar


@pytest.fixture(scope="module")
def model(orc, assets, tmp_path_factory):
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("lang") / "micro-lang")
    lm.write_lang_model(prefix + ".wtw", p + ".wtw")
    m = orc.Model(p + ".wtw")
    yield m
    m.close()


def test_mel_generator_is_pinned():
    mel = lm.lang_mels(3)
    assert mel.shape == (3, 80, 200) and mel.dtype == np.float32
    assert mel.min() >= -1.0 and mel.max() <= 1.5
    rng = np.random.default_rng(lm.MEL_SEED)
    a, s = rng.uniform(-1.0, 1.0), rng.uniform(0.1, 1.5)  # drawn in that order, then the clip's normal samples
    want = np.clip(a + s * rng.standard_normal((80, 200)), -1.0, 1.5).astype(np.float32)
    assert np.array_equal(mel[0], want)
    assert np.array_equal(lm.lang_mels(32)[:3], mel)  # a shorter batch is a prefix of the longer one


def test_language_rows_are_scaled(assets, tmp_path):
    sys.path.insert(0, os.path.join(lm.ROOT, "tools"))
    from wtw import read_wtw
    prefix, _ = assets("micro")
    dst = str(tmp_path / "m.wtw")
    lm.write_lang_model(prefix + ".wtw", dst)
    dims, t = read_wtw(dst)
    E = np.asarray(t["decoder.token_embedding.weight"])
    assert dict(dims)["n_vocab"] == lm.N_VOCAB and E.shape[0] == lm.N_VOCAB
    rms = np.sqrt((E.astype(np.float64) ** 2).mean(axis=1))
    bg = np.median(rms)
    lang = rms[lm.LANG_LO:lm.LANG_LO + lm.N_LANG]
    assert np.all(lang > 400 * bg) and np.all(rms[:lm.N_ACTIVE] > 400 * bg)  # x 40 / 0.05 = 800 against the background
    assert rms[lm.LANG_LO + lm.N_LANG] < 3 * bg and rms[lm.LANG_LO - 1] < 3 * bg  # translate and sot stay background rows


def test_fixture_languages_and_gaps(model):
    mel = lm.lang_mels()
    langs, gaps = [], []
    for b in range(lm.N_CLIPS):
        _, lang, gap = lm.oracle_language(model, model.encode(mel[b]))
        langs.append(lang)
        gaps.append(gap)
    print("languages", langs, "smallest gap", min(gaps), "median", float(np.median(gaps)))
    assert langs == lm.EXPECT_LANGS
    assert set(langs) == {87, 94}
    assert abs(min(gaps) - 0.0703) < 5e-4 and abs(float(np.median(gaps)) - 2.39) < 5e-3
    assert min(gaps) > 100 * DECISION_MARGIN  # every clip is decisive


def test_greedy_steps_are_decisive(model):
    # the 32 clips of the fixture behind their own prompt, and 8 clips of the uniform generator of test_gpu_beam.py
    mel = lm.lang_mels()
    margins = []
    for b in range(lm.N_CLIPS):
        _, m = lm.oracle_decode(model, model.encode(mel[b]), lm.EXPECT_LANGS[b])
        margins.append(m)
    print("fixture clips: smallest step margin", min(margins))
    assert min(margins) > 0.02  # measured 0.0225
    rng = np.random.default_rng(1234)
    um = rng.uniform(-1.0, 1.5, size=(8, 80, 200)).astype(np.float32)
    first, later = [], []
    for b in range(8):
        enc = model.encode(um[b])
        _, lang, gap = lm.oracle_language(model, enc)
        assert gap > 100 * DECISION_MARGIN
        _, logits = model.decode_greedy(enc, lm.prompt_for(lang), 30, lm.EOT, True, True, 8, True)
        g = [lm.top_two_gap(logits[s]) for s in range(logits.shape[0])]
        first.append(g[0])
        later.append(min(g[1:]))
    print("uniform clips: first step", min(first), "later steps", min(later))
    assert min(first) > 0.1  # measured 0.1105
    assert min(later) > 0.195  # measured 18.7
