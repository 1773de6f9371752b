"""Spoken-language detection and the per-clip automatic language (option "language" = -1) on the
GPU: the language_head kernel against float64 numpy, detection and the automatic decode against the CPU oracle on the
language model of tests/lang_model.py, the pipelined path, the bf16 storage mode and the option surface.  Without the
feature set_option("language", -1) is WT_ERR_INVALID_ARG and the new symbols do not exist, so every test here fails."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lang_model as lm  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = 4, 1
# the project's logits bar is 1e-4: a language probability is then within a factor e^{+-2e-4}
P_TOL = 3e-4
GAP = 2e-4  # an oracle decision closer than this is not asserted
# language_head against float64: fp32 LayerNorm, 99 dot products over d <= 384 and an fp32 softmax.  Measured largest
# |p - p64| over every case of test_kernel_against_float64: 1.55e-7 (a few ulp of a probability near 1)
KERNEL_P_TOL = 6e-7  # under 4 x the measured value, inside the 3e-6 that an fp32 softmax of 99 terms allows
MICRO_PROMPT = [3, 5, 7, 11]


def code_of(exc):
    return {"WT_ERR_UNSUPPORTED": UNSUPPORTED, "WT_ERR_INVALID_ARG": INVALID}.get(str(exc.value).split(":")[0])


@pytest.fixture(scope="module")
def lang_assets(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("lang") / "micro-lang")
    lm.write_lang_model(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def ref(orc, lang_assets):
    """The CPU oracle over the 32 clips, computed once: language logits, language, gap, and the greedy ids behind the
    clip's own prompt with their smallest step margin."""
    model = orc.Model(lang_assets[0] + ".wtw")
    mel = lm.lang_mels()
    out = {"mel": mel, "z": [], "lang": [], "gap": [], "ids": [], "margin": []}
    for b in range(lm.N_CLIPS):
        enc = model.encode(mel[b])
        z, lang, gap = lm.oracle_language(model, enc)
        ids, margin = lm.oracle_decode(model, enc, lang)
        for k, v in zip(("z", "lang", "gap", "ids", "margin"), (z, lang, gap, ids, margin)):
            out[k].append(v)
    model.close()
    return out


@pytest.fixture(scope="module")
def tap_eng(pkg, assets):
    prefix, vocab = assets("micro")
    eng = pkg.Engine(prefix, vocab, True)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------ 1. the kernel ---

LANG_LO_TAP = 7  # the tap's table: rows before and after the language rows hold NaN


def head_case(d, n_lang, rows, part, seed=0):
    rng = np.random.default_rng(1000 * d + 10 * n_lang + rows + (5 if part else 0) + seed)
    x = (rng.standard_normal((rows, d)) * 1.5 + 0.3).astype(np.float32)
    xp = (rng.standard_normal((rows, d)) * 0.5).astype(np.float32) if part else None
    g = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    E = np.full((LANG_LO_TAP + n_lang + 2, d), np.nan, np.float32)
    E[LANG_LO_TAP:LANG_LO_TAP + n_lang] = (rng.standard_normal((n_lang, d)) * 2.0 / np.sqrt(d)).astype(np.float32)
    return x, xp, g, b, E


def head_ref(x, xp, g, b, E, n_lang):
    """float64: (probs [rows][n_lang], logits)"""
    r = x.astype(np.float64) + (xp.astype(np.float64) if xp is not None else 0.0)
    mu = r.mean(axis=1, keepdims=True)
    var = ((r - mu) ** 2).mean(axis=1, keepdims=True)
    y = (r - mu) / np.sqrt(var + 1e-5) * g.astype(np.float64) + b.astype(np.float64)
    z = y @ E[LANG_LO_TAP:LANG_LO_TAP + n_lang].astype(np.float64).T
    return np.stack([lm.softmax64(zz) for zz in z]), z


@pytest.mark.parametrize("part", [False, True])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n_lang", [99, 5])
@pytest.mark.parametrize("d", [64, 128, 384])  # 128 is the micro model's decoder width, 384 tiny's
def test_kernel_against_float64(tap_eng, d, n_lang, rows, part):
    x, xp, g, b, E = head_case(d, n_lang, rows, part)
    ids = np.arange(rows * 6, dtype=np.int64).reshape(rows, 6) + 100
    probs, lang, prob, ids_out = tap_eng.dbg_language_head(x, g, b, E, LANG_LO_TAP, n_lang, xpart=xp, ids=ids)
    want, z = head_ref(x, xp, g, b, E, n_lang)
    err = float(np.abs(probs.astype(np.float64) - want).max())
    print(f"d {d} n_lang {n_lang} rows {rows} part {part}: max |p - p64| = {err:.3e}")
    assert np.all(np.isfinite(probs))
    assert err <= KERNEL_P_TOL
    assert np.all(np.abs(probs.astype(np.float64).sum(axis=1) - 1.0) <= 1e-5)
    for r in range(rows):
        if lm.top_two_gap(z[r]) > 1e-4:  # (these random rows sit far apart; a float64 tie would not be the kernel's)
            assert lang[r] == lm.argmax_last(z[r])
        assert prob[r] == probs[r, lang[r]]
    keep = np.ones(6, bool)
    keep[1] = False
    assert np.array_equal(ids_out[:, keep], ids[:, keep])  # the id row changes at index 1 only
    assert np.array_equal(ids_out[:, 1], LANG_LO_TAP + lang.astype(np.int64))
    # without id rows nothing else changes
    probs2, lang2, prob2, none = tap_eng.dbg_language_head(x, g, b, E, LANG_LO_TAP, n_lang, xpart=xp)
    assert none is None and np.array_equal(probs2, probs) and np.array_equal(lang2, lang) and np.array_equal(prob2, prob)


@pytest.mark.parametrize("d,n_lang,pair", [(128, 99, (3, 70)), (128, 99, (2, 66)), (384, 99, (97, 98)), (64, 5, (1, 4)),
                                           (128, 99, (0, 98))])
def test_kernel_ties_go_to_the_larger_id(tap_eng, d, n_lang, pair):
    # two identical embedding rows above every other logit: (3, 70) and (0, 98) sit in different lanes of the softmax
    # wavefront, (2, 66) in one lane, (97, 98) in neighbouring wavefronts of the dot products
    x, xp, g, b, E = head_case(d, n_lang, 2, False, seed=77)
    _, z = head_ref(x, xp, g, b, E, n_lang)
    lo, hi = pair
    for r in range(2):
        Er = E.copy()
        top = int(np.argmax(z[r]))
        assert z[r][top] > 0
        Er[LANG_LO_TAP + lo] = Er[LANG_LO_TAP + hi] = 1.5 * E[LANG_LO_TAP + top]
        ids = np.zeros((2, 4), np.int64)
        probs, lang, prob, ids_out = tap_eng.dbg_language_head(x, g, b, Er, LANG_LO_TAP, n_lang, ids=ids)
        assert probs[r, lo] == probs[r, hi] and probs[r, hi] == probs[r].max()
        assert lang[r] == hi and ids_out[r, 1] == LANG_LO_TAP + hi


@pytest.mark.parametrize("d,part", [(128, False), (384, True)])
def test_kernel_row_is_independent_of_the_grid(tap_eng, d, part):
    x, xp, g, b, E = head_case(d, 99, 3, part, seed=5)
    p3, l3, q3, _ = tap_eng.dbg_language_head(x, g, b, E, LANG_LO_TAP, 99, xpart=xp)
    p1, l1, q1, _ = tap_eng.dbg_language_head(x[2:3], g, b, E, LANG_LO_TAP, 99, xpart=xp[2:3] if part else None)
    assert p1.tobytes() == p3[2:3].tobytes() and l1[0] == l3[2] and q1.tobytes() == q3[2:3].tobytes()


def test_kernel_forced_language_and_bad_arguments(pkg, tap_eng):
    x, xp, g, b, E = head_case(128, 99, 3, False, seed=9)
    ids = np.zeros((3, 4), np.int64)
    free = tap_eng.dbg_language_head(x, g, b, E, LANG_LO_TAP, 99)
    probs, lang, prob, ids_out = tap_eng.dbg_language_head(x, g, b, E, LANG_LO_TAP, 99, ids=ids, forced_lang=41)
    assert np.array_equal(probs, free[0])  # the probabilities are the detected ones
    assert list(lang) == [41] * 3 and np.array_equal(prob, probs[:, 41]) and list(ids_out[:, 1]) == [LANG_LO_TAP + 41] * 3
    for kw in ({"lang_lo": E.shape[0] - 98}, {"n_lang": 0}, {"n_lang": 129}, {"forced_lang": 99}, {"lang_lo": -1}):
        a = {"lang_lo": LANG_LO_TAP, "n_lang": 99, "forced_lang": -1}
        a.update(kw)
        with pytest.raises(pkg.WtError) as e:  # a range outside the table never reaches the kernel
            tap_eng.dbg_language_head(x, g, b, E, a["lang_lo"], a["n_lang"], forced_lang=a["forced_lang"])
        assert code_of(e) == INVALID


# --------------------------------------------------------------------------------- 2. detection vs oracle ---

@pytest.fixture(scope="module")
def eng(pkg, lang_assets):
    e = pkg.Engine(lang_assets[0], lang_assets[1], True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def detected(eng, ref):
    """detect_language over the 32 clips, once."""
    return eng.detect_language(ref["mel"])


def test_detection_against_the_oracle(eng, ref, detected):
    assert eng.language_count() == lm.N_LANG
    assert eng.vocab_info()["translate"] == lm.LANG_LO + lm.N_LANG
    for batch in (32, 1, 3):
        lang, probs = detected if batch == 32 else eng.detect_language(ref["mel"][:batch])
        assert probs.shape == (batch, lm.N_LANG)
        worst = 0.0
        for b in range(batch):
            want = lm.softmax64(ref["z"][b])
            worst = max(worst, float(np.abs(probs[b].astype(np.float64) - want).max()))
            if ref["gap"][b] > GAP:
                assert lang[b] == ref["lang"][b], (batch, b, lang[b], ref["lang"][b], ref["gap"][b])
        print(f"batch {batch}: max |p - p_oracle| = {worst:.3e}")
        assert worst <= P_TOL
    assert all(g > GAP for g in ref["gap"])  # the fixture: all 32 clips are asserted
    assert set(int(x) for x in detected[0]) == {87, 94}
    dev = eng.device_array(ref["mel"][:5])
    lang_d, probs_d = eng.detect_language_dev(dev.data_ptr(), 5)
    dev.free()
    assert np.array_equal(lang_d, detected[0][:5])
    # detection does not depend on the decoding options it does not use
    eng.set_option("beam_size", 4)
    eng.set_prompt([lm.SOT, lm.LANG_LO, lm.TRANSCRIBE])
    lang_b, probs_b = eng.detect_language(ref["mel"][:3])
    eng.set_prompt([])
    eng.set_option("beam_size", 1)
    assert np.array_equal(lang_b, detected[0][:3])


# -------------------------------------------------------------------------------------- 3. automatic decode ---

def explicit_ids(pkg, lang_assets, mel, lang, **opts):
    """ids of a fresh engine that decodes the whole batch with ONE given language."""
    e = pkg.Engine(lang_assets[0], lang_assets[1], True)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_option("language", int(lang))
    out = e.encdec_tokens_batch(mel)
    e.close()
    return out


def check_against_oracle(ids, n, ref, clips):
    for i, b in enumerate(clips):
        if ref["gap"][b] > GAP and ref["margin"][b] > GAP:
            assert [int(t) for t in ids[i, : n[i]]] == ref["ids"][b], (b, ref["margin"][b])


@pytest.fixture(scope="module")
def auto32(pkg, lang_assets, ref):
    """The synchronous automatic decode of the 32 clips on an engine of its own: (ids, n, languages, probabilities)."""
    e = pkg.Engine(lang_assets[0], lang_assets[1], True)
    e.set_option("language", pkg.WT_LANGUAGE_AUTO)
    assert e.get_option("language") == -1
    ids, n = e.encdec_tokens_batch(ref["mel"])
    lang, prob = e.last_languages()
    e.close()
    return ids, n, lang, prob


def test_auto_decode(pkg, lang_assets, ref, detected, auto32):
    ids, n, lang, prob = auto32
    assert np.array_equal(lang, detected[0])
    assert np.abs(prob - detected[1][np.arange(32), lang]).max() <= 1e-6
    assert np.array_equal(ids[:, 1], lm.LANG_LO + lang.astype(np.int64))
    assert np.all(ids[:, 0] == lm.SOT) and np.all(ids[:, 2] == lm.TRANSCRIBE) and np.all(ids[:, 3] == lm.NOTIMESTAMPS)
    for L in sorted(set(int(x) for x in lang)):
        ids_L, n_L = explicit_ids(pkg, lang_assets, ref["mel"], L)
        sel = np.nonzero(lang == L)[0]
        assert np.array_equal(ids[sel], ids_L[sel]) and np.array_equal(n[sel], n_L[sel]), L
    check_against_oracle(ids, n, ref, range(32))
    assert all(m > GAP for m in ref["margin"])  # the fixture: every clip is compared


def test_auto_graphs_and_eager_agree(pkg, lang_assets, ref, auto32):
    e = pkg.Engine(lang_assets[0], lang_assets[1], True)
    e.set_option("language", -1)
    a = e.encdec_tokens_batch(ref["mel"])  # eager, then captured
    b = e.encdec_tokens_batch(ref["mel"])  # replayed
    lb = e.last_languages()
    e.set_option("use_graphs", 0)
    c = e.encdec_tokens_batch(ref["mel"])
    lc = e.last_languages()
    e.close()
    for x in (a, b, c):
        assert np.array_equal(x[0], auto32[0]) and np.array_equal(x[1], auto32[1])
    assert np.array_equal(lb[0], lc[0]) and np.array_equal(lb[1], lc[1]) and np.array_equal(lb[0], auto32[2])


@pytest.mark.parametrize("absorb", [0, 1])
def test_auto_both_cross_attention_forms(pkg, lang_assets, ref, auto32, absorb):
    clips = [0, 22, 24]  # two languages in a batch of 3
    e = pkg.Engine(lang_assets[0], lang_assets[1], True)
    e.set_option("cross_absorb", absorb)
    e.set_option("language", -1)
    ids, n = e.encdec_tokens_batch(ref["mel"][clips])
    lang, _ = e.last_languages()
    e.close()
    assert list(lang) == [ref["lang"][b] for b in clips]
    check_against_oracle(ids, n, ref, clips)
    assert np.array_equal(ids, auto32[0][clips]) and np.array_equal(n, auto32[1][clips])


def test_auto_long_audio_and_pcm_entry_points(pkg, lang_assets):
    e = pkg.Engine(lang_assets[0], lang_assets[1], True)
    rng = np.random.default_rng(42)
    pcm = (0.1 * rng.standard_normal((2, e.pcm_len))).astype(np.float32)
    pcm[1] *= 4.0
    e.set_option("language", -1)
    text = e.transcribe_long(pcm.reshape(-1))
    lang, prob = e.last_languages()
    assert lang.shape == (2,)
    per = []
    for w in range(2):
        per.append(e.transcribe(pcm[w]))
        l1, p1 = e.last_languages()
        assert l1.shape == (1,) and l1[0] == lang[w] and abs(p1[0] - prob[w]) <= 1e-6
        ld, pd = e.detect_language_pcm(pcm[w])
        assert ld == lang[w] and abs(pd - prob[w]) <= 1e-6
    assert text == "\n".join(per)
    mel = e.logmel_batch(pcm)
    dev = e.device_array(pcm)
    ids_t, n_t = e.transcribe_tokens_batch_dev(dev.data_ptr(), 2)
    dev.free()
    ids_m, n_m = e.encdec_tokens_batch(mel)
    assert np.array_equal(ids_t, ids_m) and np.array_equal(n_t, n_m)
    assert list(ids_m[:, 1] - lm.LANG_LO) == list(lang)
    e.close()


# ------------------------------------------------------------------------------------------- 4. pipelined ---

def test_auto_pipelined(pkg, lang_assets, ref, auto32):
    e = pkg.Engine(lang_assets[0], lang_assets[1], True)
    e.set_option("language", -1)
    small = e.encdec_tokens_batch(ref["mel"][:3])  # the synchronous ids of the short batch
    assert np.array_equal(small[0], auto32[0][:3])
    devs = [e.device_array(ref["mel"][8 * k: 8 * k + 8]) for k in range(4)] + [e.device_array(ref["mel"][:3])]
    for k in range(4):
        e.pipeline_submit_dev(devs[k].data_ptr(), 8)  # paired chains: rows = 2 x 8
    e.pipeline_submit_dev(devs[4].data_ptr(), 3)
    with pytest.raises(pkg.WtError):  # synchronous state only
        e.last_languages()
    for k in range(4):
        ids, n = e.pipeline_collect()
        assert np.array_equal(ids, auto32[0][8 * k: 8 * k + 8]) and np.array_equal(n, auto32[1][8 * k: 8 * k + 8]), k
        assert np.array_equal(ids[:, 1] - lm.LANG_LO, auto32[2][8 * k: 8 * k + 8])
    ids, n = e.pipeline_collect()
    assert np.array_equal(ids, small[0]) and np.array_equal(n, small[1])
    for d in devs:
        d.free()
    e.close()


# ------------------------------------------------------------------------------------------------ 5. bf16 ---

def test_auto_bf16_is_self_consistent(pkg, lang_assets, ref):
    # no oracle tolerance is invented for the bf16 storage mode: the automatic decode must equal the explicit decode
    # with the language the bf16 engine itself detected, clip by clip
    e = pkg.Engine(lang_assets[0], lang_assets[1], True)
    e.set_option("bf16", 1)
    det, _ = e.detect_language(ref["mel"])
    e.set_option("language", -1)
    ids, n = e.encdec_tokens_batch(ref["mel"])
    lang, _ = e.last_languages()
    e.close()
    assert np.array_equal(lang, det) and np.array_equal(ids[:, 1], lm.LANG_LO + lang.astype(np.int64))
    for L in sorted(set(int(x) for x in lang)):
        ids_L, n_L = explicit_ids(pkg, lang_assets, ref["mel"], L, bf16=1)
        sel = np.nonzero(lang == L)[0]
        assert np.array_equal(ids[sel], ids_L[sel]) and np.array_equal(n[sel], n_L[sel]), L


# --------------------------------------------------------------------------------------------- 6. surface ---

def test_option_surface_and_scope_cuts(pkg, assets, lang_assets, ref, auto32):
    import ctypes
    L = pkg.lib()
    e = pkg.Engine(lang_assets[0], lang_assets[1], True)
    mel = ref["mel"][:2]
    assert e.get_option("language") == 2
    for bad in (-2, 100):
        with pytest.raises(pkg.WtError) as x:
            e.set_option("language", bad)
        assert code_of(x) == INVALID
    assert e.get_option("language") == 2
    e.encdec_tokens_batch(mel)
    assert L.wt_last_languages(e.handle, None, None, 0) == -INVALID  # the last decode did not detect
    with pytest.raises(pkg.WtError):
        e.last_languages()

    def unsupported(fn):
        with pytest.raises(pkg.WtError) as x:
            fn()
        assert code_of(x) == UNSUPPORTED, str(x.value)
        assert "language" in str(x.value)  # wt_last_error says why

    e.set_option("language", -1)
    want = e.encdec_tokens_batch(mel)
    assert np.array_equal(want[0], auto32[0][:2])
    e.set_option("beam_size", 4)
    unsupported(lambda: e.encdec_tokens_batch(mel))
    e.set_option("beam_size", 1)
    e.set_prompt([lm.SOT, lm.LANG_LO + 2, lm.TRANSCRIBE, lm.NOTIMESTAMPS])
    unsupported(lambda: e.encdec_tokens_batch(mel))
    dev = e.device_array(mel)
    unsupported(lambda: e.pipeline_submit_dev(dev.data_ptr(), 2))
    e._submitted = []
    e.set_prompt([])
    forced = np.zeros((2, 32), np.int64)
    forced[:, :4] = lm.prompt_for(2)
    assert L.wt_dbg_set_forced_ids(e.handle, forced.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 2) == 0
    unsupported(lambda: e.encdec_tokens_batch(mel))
    unsupported(lambda: e.pipeline_submit_dev(dev.data_ptr(), 2))
    e._submitted = []
    dev.free()
    assert L.wt_dbg_set_forced_ids(e.handle, None, 0) == 0
    again = e.encdec_tokens_batch(mel)  # everything restored: the engine is usable and gives the same result
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    e.close()

    # engines without language tokens: the Monolith graph forces <|en|>, English-only ids, the 1024-entry micro vocabulary
    mono = pkg.Engine(lang_assets[0], lang_assets[1], True, pkg.EngineType.Monolith)
    unsupported(lambda: mono.set_option("language", -1))
    assert mono.get_option("language") == 0
    mono.encdec_tokens_batch(mel)
    mono.close()
    eng_only = pkg.Engine(lang_assets[0], lang_assets[1], False)
    unsupported(lambda: eng_only.set_option("language", -1))
    unsupported(lambda: eng_only.detect_language(mel))
    assert L.wt_language_count(eng_only.handle) == -UNSUPPORTED
    eng_only.close()
    prefix, vocab = assets("micro")
    micro = pkg.Engine(prefix, vocab, True)
    micro.set_prompt(MICRO_PROMPT)
    unsupported(lambda: micro.set_option("language", -1))
    unsupported(lambda: micro.detect_language(mel))
    with pytest.raises(pkg.WtError):
        micro.language_count()
    micro.encdec_tokens_batch(mel)
    micro.close()


@pytest.mark.parametrize("batch", [8, 40])
def test_defaults_untouched(pkg, lang_assets, batch):
    rng = np.random.default_rng(99)
    mel = rng.uniform(-1.0, 1.5, size=(batch, 80, 200)).astype(np.float32)
    fresh = pkg.Engine(lang_assets[0], lang_assets[1], True)  # never sees the option
    ids_ref, n_ref = fresh.encdec_tokens_batch(mel)
    fresh.close()
    e = pkg.Engine(lang_assets[0], lang_assets[1], True)
    e.set_option("language", -1)
    ids_a, n_a = e.encdec_tokens_batch(mel)
    assert np.all(ids_a[:, 1] >= lm.LANG_LO) and np.all(ids_a[:, 1] < lm.LANG_LO + lm.N_LANG)
    e.set_option("language", 2)
    ids, n = e.encdec_tokens_batch(mel)
    e.close()
    assert np.array_equal(ids, ids_ref) and np.array_equal(n, n_ref)
