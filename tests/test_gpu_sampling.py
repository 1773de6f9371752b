"""Temperature sampling and fall-back (options temperature, seed, temperature_fallback with max_positions; DESIGN.md
section 19) on the GPU against tests/sample_ref.py over the CPU oracle, on the fixtures of tests/sample_model.py
(tests/test_sample_reference.py pins what the reference gives on them).  Without the feature
set_option("temperature", ...) fails and so does every test here.

Ids and counts must equal the reference up to each clip's first indecisive step (sample_model.compared_steps: the kernel's
key bar plus twice the logits bar over T); the fixtures' clips are decisive over their whole path, so that is all of
them.  Token log-probabilities stay within section 15's bound of the reference."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sample_model as smp  # noqa: E402
import sample_ref as sr  # noqa: E402
import scores_model as sm  # noqa: E402
import ts_ref  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
TOKEN_BOUND = 1.1e-4  # section 15: five times the largest measured |lp - reference lp| of a token
worst = {"lp": 0.0}


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def models(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    d = tmp_path_factory.mktemp("sampling")
    ts, plain = str(d / "micro-scores-ts"), str(d / "micro-scores-plain")
    sm.write_ts_model(prefix + ".wtw", ts + ".wtw")
    sm.write_plain_model(prefix + ".wtw", plain + ".wtw")
    return {"ts": (ts, vocab), "plain": (plain, vocab)}


@pytest.fixture(scope="module")
def mels():
    out = {"ts": sm.ts_mels(), "plain": sm.plain_mels()}
    for m in out.values():
        m.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def ref(orc, models, mels):
    """The reference rows, each computed once on demand and never changed."""
    r = smp.Reference(orc, {k: v[0] for k, v in models.items()}, mels)
    yield r
    r.close()


def new_engine(pkg, models, mode, positions, **options):
    eng = pkg.Engine(models[mode][0], models[mode][1], True)
    eng.set_option("max_positions", positions)
    eng.set_option("timestamps", 1 if mode == "ts" else 0)
    eng.set_option("scores", 1)
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


def n0_of(mode):
    return len(sm.TS_PROMPT if mode == "ts" else sm.PLAIN_PROMPT)


def decode(eng, mel):
    ids, n = eng.encdec_tokens_full(np.ascontiguousarray(mel))
    return ids, n, eng.last_scores(), eng.last_token_logprobs(ids.shape[1])


def gen_text(eng, ids_row, n, n0):
    return eng.decode_bytes(np.array([i for i in ids_row[n0:n] if i < sm.EOT], np.int64), True)


def check(eng, got, rows, n0, milli):
    """Ids, counts, token log-probabilities, scores and the decode info against reference rows."""
    ids, n, sc, lp = got
    info = eng.last_decode_info()
    assert ids.shape[0] == len(rows) == sc.size == lp.shape[0] == info.size
    for row, r in enumerate(rows):
        k = smp.compared_steps(r, milli)
        assert k == r["n"] or k >= 1, row
        assert [int(x) for x in ids[row, : n0 + k]] == r["ids"][: n0 + k], row
        have = lp[row, n0: n0 + k].astype(np.float64)
        err = float(np.abs(have - np.asarray(r["lps"][:k], np.float64)).max())
        worst["lp"] = max(worst["lp"], err)
        assert err <= TOKEN_BOUND, (row, err)
        assert abs(sc["no_speech_prob"][row] - r["no_speech_prob"]) <= (TOKEN_BOUND + 2.0 ** -23) * r["no_speech_prob"]
        assert info["temperature_milli"][row] == milli and info["attempts"][row] == 1 and info["needs_fallback"][row] == 0
        if k < r["n"]:
            continue  # an indecisive step: the rest of the row may differ
        assert n[row] == len(r["ids"]) and sc["n_generated"][row] == r["n"]
        assert not lp[row, :n0].any() and not lp[row, n[row]:].any()
        assert abs(sc["sum_logprob"][row] - r["sum"]) <= TOKEN_BOUND * r["n"] + abs(r["sum"]) * 2.0 ** -23
        assert abs(sc["avg_logprob"][row] - r["avg"]) <= TOKEN_BOUND + abs(r["avg"]) * 2.0 ** -23
        want = np.float32(sr.compression_ratio(gen_text(eng, ids[row], n[row], n0)))
        assert info["compression_ratio"][row].tobytes() == want.tobytes()  # bit-equal to Python's on the same text


@pytest.mark.parametrize("milli", smp.TEMPS)
@pytest.mark.parametrize("mode", ["ts", "plain"])
def test_fixed_temperature_equals_the_reference(pkg, models, mels, ref, mode, milli):
    """5 rows and 1 row over the long decode, eager, replayed, replayed under another seed, and the cut at P_SHORT."""
    P = sm.P_LONG if mode == "ts" else sm.P_PLAIN
    n0, mel = n0_of(mode), mels[mode]
    eng = new_engine(pkg, models, mode, P, temperature=milli, seed=smp.SEED)
    rows = [ref.row(mode, b, b, milli, smp.SEED, P) for b in range(5)]
    first = decode(eng, mel[:5])          # eager, then captured
    check(eng, first, rows, n0, milli)
    again = decode(eng, mel[:5])          # the segment graphs replayed: the same bits
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    eng.set_option("seed", smp.OTHER_SEED)  # the same graphs under another seed: the reference of THAT seed
    other = decode(eng, mel[:2])
    check(eng, other, [ref.row(mode, b, b, milli, smp.OTHER_SEED, P) for b in range(2)], n0, milli)
    again = decode(eng, mel[:2])
    for a, b in zip(other, again):
        assert a.tobytes() == b.tobytes()
    eng.set_option("seed", smp.SEED)
    check(eng, decode(eng, mel[3:4]), [ref.row(mode, 3, 0, milli, smp.SEED, P)], n0, milli)  # one row: clip index 0
    eng.set_option("max_positions", smp.P_SHORT)  # the cut inside the second segment
    check(eng, decode(eng, mel[:5]), [ref.row(mode, b, b, milli, smp.SEED, smp.P_SHORT) for b in range(5)], n0, milli)
    eng.set_option("use_graphs", 0)
    check(eng, decode(eng, mel[:5]), [ref.row(mode, b, b, milli, smp.SEED, smp.P_SHORT) for b in range(5)], n0, milli)
    eng.close()


@pytest.mark.parametrize("mode,milli,forms", [("ts", 200, True), ("plain", 1000, True), ("ts", 1000, False), ("plain", 200, False)])
def test_64_rows_both_cross_attention_forms_and_eager(pkg, models, mels, ref, mode, milli, forms):
    """64 rows (every one its own clip index, so every one its own reference decode) at both temperatures in both modes;
    two of the four also on the cached cross-attention and eager."""
    n0, mel = n0_of(mode), mels[mode]
    pick = [b % mel.shape[0] for b in range(64)]
    mel64 = np.ascontiguousarray(mel[pick])
    rows = [ref.row(mode, pick[b], b, milli, smp.SEED, smp.P_SHORT) for b in range(64)]
    eng = new_engine(pkg, models, mode, smp.P_SHORT, temperature=milli, seed=smp.SEED)
    assert eng.get_option("cross_absorb_active") == 1
    g64 = decode(eng, mel64)
    check(eng, g64, rows, n0, milli)
    for a, b in zip(g64, decode(eng, mel64)):  # replay
        assert a.tobytes() == b.tobytes()
    if not forms:
        eng.close()
        return
    eng.set_option("cross_absorb", 0)
    check(eng, decode(eng, mel64), rows, n0, milli)
    eng.set_option("use_graphs", 0)
    check(eng, decode(eng, mel64), rows, n0, milli)
    eng.set_option("cross_absorb", 1)
    check(eng, decode(eng, mel64), rows, n0, milli)
    eng.close()


@pytest.mark.parametrize("mode", ["ts", "plain"])
def test_zero_temperature_on_the_sampling_path_is_the_greedy_decode(pkg, models, mels, mode):
    """Fall-back enabled with thresholds that never trigger: the sampling kernels at T = 0 give the option-off bytes."""
    P = sm.P_LONG if mode == "ts" else sm.P_PLAIN
    mel = mels[mode]
    eng = new_engine(pkg, models, mode, P)
    off = decode(eng, mel)
    with pytest.raises(pkg.WtError) as e:
        eng.last_decode_info()  # that decode neither sampled nor fell back
    assert status_of(e) == INVALID
    for k, v in (("temperature_fallback", 1), ("compression_ratio_threshold", 0), ("logprob_threshold", -1000000), ("seed", 77)):
        eng.set_option(k, v)
    on = decode(eng, mel)
    for a, b in zip(off, on):
        assert a.tobytes() == b.tobytes()
    info = eng.last_decode_info()
    assert (info["attempts"] == 1).all() and (info["temperature_milli"] == 0).all() and not info["needs_fallback"].any()
    if mode == "ts":
        segs = eng.last_segments()
        want = []
        for b in range(on[0].shape[0]):
            want += ts_ref.segments(on[0][b, : on[1][b]], n0_of(mode), sm.EOT, sm.BEG, clip=b)
        assert [tuple(int(x) for x in s) for s in segs] == want
    eng.set_option("temperature_fallback", 0)
    again = decode(eng, mel)  # off again: the greedy kernels, the same bytes, and no decode info
    for a, b in zip(off, again):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(pkg.WtError) as e:
        eng.last_decode_info()
    assert status_of(e) == INVALID
    eng.close()


def test_fallback_equals_the_reference_loop(pkg, models, mels, ref):
    """The pinned fixture: clips accepted at T = 0, at an intermediate temperature, kept by the silence exemption, and
    clips that exhaust the schedule; ids, counts, scores, decode info and segments are the merged result's."""
    fb, n0, mel = smp.FB, len(sm.TS_PROMPT), mels["ts"]
    eng = new_engine(pkg, models, "ts", smp.P_SHORT, temperature_fallback=1, **fb)
    rows = ref.fallback(lambda ids, n_prompt: gen_text(eng, np.asarray(ids), len(ids), n_prompt))
    assert {r["attempts"] for r in rows} == {1, 2, 3}
    for attempt in range(2):  # eager + captured, then replayed
        ids, n, sc, lp = decode(eng, mel)
        info = eng.last_decode_info()
        assert eng.timings().decoder_steps > smp.P_SHORT  # summed over the attempts
        for b, r in enumerate(rows):
            assert [int(x) for x in ids[b, : n[b]]] == r["ids"], b
            assert (int(info["attempts"][b]), int(info["temperature_milli"][b]), int(info["needs_fallback"][b])) == \
                (r["attempts"], r["temperature_milli"], int(r["needs_fallback"])), b
            assert info["compression_ratio"][b].tobytes() == np.float32(r["compression_ratio"]).tobytes()
            err = float(np.abs(lp[b, n0: n[b]].astype(np.float64) - np.asarray(r["lps"], np.float64)).max())
            worst["lp"] = max(worst["lp"], err)
            assert err <= TOKEN_BOUND and not lp[b, n[b]:].any()
            assert sc["n_generated"][b] == r["n"]
            assert abs(sc["avg_logprob"][b] - r["avg"]) <= TOKEN_BOUND + abs(r["avg"]) * 2.0 ** -23
            assert abs(sc["no_speech_prob"][b] - r["no_speech_prob"]) <= (TOKEN_BOUND + 2.0 ** -23) * r["no_speech_prob"]
        segs, seg_scores = eng.last_segments(with_scores=True)
        want = []
        for b, r in enumerate(rows):
            want += ts_ref.segments(r["ids"], n0, sm.EOT, sm.BEG, clip=b)
        assert [tuple(int(x) for x in s) for s in segs] == want
        for s, got in zip(segs, seg_scores):
            b, i0, cnt = int(s["clip"]), int(s["id_begin"]), int(s["id_count"])
            assert abs(got - float(lp[b, i0: i0 + cnt].astype(np.float64).mean())) <= 1e-6 * max(1.0, abs(got))
    # a subset of the clips in another order: every clip's result depends on its own index in the call alone
    sub = [7, 2, 4]
    rows3 = ref.fallback(lambda ids, n_prompt: gen_text(eng, np.asarray(ids), len(ids), n_prompt), clips=sub)
    ids, n, _, _ = decode(eng, mel[sub])
    info = eng.last_decode_info()
    for b, r in enumerate(rows3):
        assert [int(x) for x in ids[b, : n[b]]] == r["ids"] and int(info["attempts"][b]) == r["attempts"]
    eng.close()


def test_text_entry_points_and_long_audio(pkg, orc, models):
    """Windows of noise through the text entry points: a window's text is the reference's under its index in the file
    (wt_transcribe_long_pcm) or under index 0 (wt_transcribe_pcm), and with fall-back on the texts, scores and decode
    info are those of the token call on the same log-mel."""
    milli = 1000
    eng = new_engine(pkg, models, "ts", smp.P_SHORT, temperature=milli, seed=smp.SEED)
    rng = np.random.default_rng(42)
    pcm = (0.1 * rng.standard_normal((2, eng.pcm_len))).astype(np.float32)
    mel = eng.logmel_batch(pcm)
    r = smp.Reference(orc, {"ts": models["ts"][0]}, {"ts": mel})
    n0 = len(sm.TS_PROMPT)
    rows = [r.row("ts", b, b, milli, smp.SEED, smp.P_SHORT) for b in range(2)]
    alone = r.row("ts", 1, 0, milli, smp.SEED, smp.P_SHORT)  # window 1 as the only clip of a call
    assert all(smp.compared_steps(x, milli) == x["n"] for x in rows + [alone])
    assert alone["ids"] != rows[1]["ids"]
    lines = eng.transcribe_long(pcm.reshape(-1)).split("\n")
    assert lines == [eng.decode_text(np.array(x["ids"], np.int64)) for x in rows]
    info = eng.last_decode_info()
    assert info.size == 2 and (info["temperature_milli"] == milli).all()
    assert eng.transcribe(pcm[1]) == eng.decode_text(np.array(alone["ids"], np.int64))
    assert eng.transcribe(pcm[0]) == lines[0] and eng.last_decode_info().size == 1
    # two single-window calls of the token entry point give the texts of clip index 0; the batch call those of 0 and 1
    ids, n = eng.encdec_tokens_full(mel)
    assert [eng.decode_text(ids[b, : n[b]]) for b in range(2)] == lines
    r.close()
    # fall-back through the text entry points: the merged result
    # (logprob_threshold = 0 and no silence exemption: every window asks for another attempt until the schedule ends)
    for k, v in dict(smp.FB, temperature_fallback=1, logprob_threshold=0, no_speech_threshold=1000).items():
        eng.set_option(k, v)
    ids, n = eng.encdec_tokens_full(mel)
    sc, info = eng.last_scores(), eng.last_decode_info()
    assert (info["attempts"] == len(smp.FB_TEMPS)).all() and (info["temperature_milli"] == smp.FB_TEMPS[-1]).all()
    assert info["needs_fallback"].all()
    text = eng.transcribe_long(pcm.reshape(-1))
    assert text == "\n".join(eng.decode_text(ids[b, : n[b]]) for b in range(2))
    assert eng.last_scores().tobytes() == sc.tobytes() and eng.last_decode_info().tobytes() == info.tobytes()
    assert eng.transcribe(pcm[0]) == eng.decode_text(ids[0, : n[0]])
    assert eng.last_decode_info().tobytes() == info[:1].tobytes()
    assert n0 == 3
    eng.close()


def test_a_window_keeps_its_index_in_the_file_across_batches(pkg, orc, models):
    """33 windows: wt_transcribe_long_pcm decodes them as batches of 32 and 1, and the last window's text is the
    reference's under clip index 32, not 0; a token call afterwards counts its clips from 0 again."""
    milli = 1000
    eng = new_engine(pkg, models, "ts", smp.P_SHORT, temperature=milli, seed=smp.SEED)
    rng = np.random.default_rng(43)
    pcm = (0.1 * rng.standard_normal((33, eng.pcm_len))).astype(np.float32)
    mel = eng.logmel_batch(pcm)
    r = smp.Reference(orc, {"ts": models["ts"][0]}, {"ts": mel})
    want = {w: r.row("ts", w, w, milli, smp.SEED, smp.P_SHORT) for w in (0, 31, 32)}
    as_first = r.row("ts", 32, 0, milli, smp.SEED, smp.P_SHORT)
    assert all(smp.compared_steps(x, milli) == x["n"] for x in list(want.values()) + [as_first])
    assert as_first["ids"] != want[32]["ids"]
    lines = eng.transcribe_long(pcm.reshape(-1)).split("\n")
    assert len(lines) == 33
    for w, x in want.items():
        assert lines[w] == eng.decode_text(np.array(x["ids"], np.int64)), w
    info = eng.last_decode_info()
    assert info.size == 33 and (info["attempts"] == 1).all()
    ids, n = eng.encdec_tokens_full(mel[32:33])  # the clip base does not outlive the long-audio call
    assert [int(i) for i in ids[0, : n[0]]] == as_first["ids"]
    r.close()
    eng.close()


def test_refusals(pkg, models, mels):
    from conftest import DevBuf
    three = np.ascontiguousarray(mels["plain"][:3])
    eng = pkg.Engine(models["plain"][0], models["plain"][1], True)
    parent_ids, parent_n = eng.encdec_tokens_batch(three)
    keys = ("temperature", "temperature_fallback", "scores", "max_positions", "beam_size", "bf16", "language")
    defaults = (("temperature", 0), ("temperature_fallback", 0), ("scores", 0), ("max_positions", 0), ("beam_size", 1),
                ("bf16", 0), ("language", 2))

    def refused(fn, code=UNSUPPORTED, after=None):
        with pytest.raises(pkg.WtError) as e:
            fn()
        if after:
            after()
        assert status_of(e) == code, str(e.value)
        assert len(str(e.value).split(":", 1)[1].strip()) > 0  # a wt_last_error text
        keep = {k: eng.get_option(k) for k in keys}  # the engine stays usable: a default call gives the parent's ids
        for k, v in defaults:
            eng.set_option(k, v)
        ids, n = eng.encdec_tokens_batch(three)
        assert np.array_equal(ids, parent_ids) and np.array_equal(n, parent_n)
        for k in ("language", "bf16", "beam_size", "max_positions", "scores", "temperature_fallback", "temperature"):
            eng.set_option(k, keep[k])

    for key, bad in (("temperature", -1), ("temperature", 1001), ("temperature_fallback", 2), ("temperature_increment", 0),
                     ("compression_ratio_threshold", -1)):
        with pytest.raises(pkg.WtError) as e:
            eng.set_option(key, bad)
        assert status_of(e) == INVALID
    assert [eng.get_option(k) for k in ("temperature", "temperature_fallback", "temperature_increment",
                                        "compression_ratio_threshold", "seed")] == [0, 0, 200, 2400, 0]
    dev = DevBuf(three)
    pcm = np.zeros(1600, np.float32)
    for option in ("temperature", "temperature_fallback"):
        eng.set_option(option, 600 if option == "temperature" else 1)
        eng.set_option("scores", 1)
        # without max_positions: every decode call
        refused(lambda: eng.encdec_tokens_batch(three))
        refused(lambda: eng.encdec_tokens_batch_dev(dev.data_ptr(), 3))
        refused(lambda: eng.transcribe(pcm))
        refused(lambda: eng.transcribe_long(pcm))
        refused(lambda: eng.pipeline_submit_dev(dev.data_ptr(), 3))
        eng._submitted = []
        assert eng.get_option("in_flight") == 0
        # with it: whatever max_positions refuses
        eng.set_option("max_positions", sm.P_PLAIN)
        refused(lambda: eng.encdec_tokens_batch(three))                # rows of WT_MAX_IDS ids
        refused(lambda: eng.pipeline_submit_dev(dev.data_ptr(), 3))    # the pipeline
        eng._submitted = []
        eng.set_option("beam_size", 4)
        refused(lambda: eng.encdec_tokens_full(three))
        eng.set_option("beam_size", 1)
        eng.set_option("bf16", 1)
        refused(lambda: eng.encdec_tokens_full(three))
        eng.set_option("bf16", 0)
        eng.set_option("language", pkg.WT_LANGUAGE_AUTO)
        refused(lambda: eng.encdec_tokens_full(three))
        eng.set_option("language", 2)
        forced = np.zeros((3, 32), np.int64)
        forced[:, :4] = sm.PLAIN_PROMPT
        eng.set_forced_ids(forced)
        refused(lambda: eng.encdec_tokens_full(three), after=lambda: eng.set_forced_ids(None))  # (the tap would steer the default call too)
        eng.encdec_tokens_full(three)  # everything restored: a sampling call works
        assert eng.last_decode_info().size == 3
        eng.set_option("max_positions", 0)
        eng.set_option("scores", 0)
        eng.set_option(option, 0)
    # fall-back without scores
    eng.set_option("max_positions", sm.P_PLAIN)
    eng.set_option("temperature_fallback", 1)
    refused(lambda: eng.encdec_tokens_full(three))
    refused(lambda: eng.transcribe(pcm))
    eng.set_option("temperature_fallback", 0)
    eng.set_option("temperature", 600)  # a fixed temperature needs no scores
    ids, n = eng.encdec_tokens_full(three)
    info = eng.last_decode_info()
    assert info.size == 3 and (info["temperature_milli"] == 600).all() and (info["attempts"] == 1).all()
    with pytest.raises(pkg.WtError):
        eng.last_scores()
    eng.set_option("temperature", 0)
    eng.set_option("max_positions", 0)
    dev.free()
    ids, n = eng.encdec_tokens_batch(three)  # a default transcription afterwards
    assert np.array_equal(ids, parent_ids) and np.array_equal(n, parent_n)
    with pytest.raises(pkg.WtError) as e:
        eng.last_decode_info()
    assert status_of(e) == INVALID
    eng.close()


def test_zz_report():
    print("largest |lp - reference lp| per token: %.3e" % worst["lp"])
