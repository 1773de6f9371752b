"""Several samples per clip (option best_of with max_positions) on the GPU against the recorded
reference of tests/best_of_model.py (tests/golden/best_of_rows.npz: tests/best_of_ref.py over tests/sample_ref.py over
the CPU oracle; tests/test_best_of_reference.py recomputes it).  Without the feature set_option("best_of", ...) fails
and so does every test here.

On a decisive clip (best_of_model: every sample decisive over its whole path, the best two averages more than 2.2e-4
apart) the kept sample, its ids and every sample's count must equal the reference; token log-probabilities stay within
section 15's 1.1e-4 and every sample's sum within that times its count.  A clip set aside is compared up to the kept
sample's first indecisive step, and only where the engine kept the reference's sample."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import best_of_model as bm  # noqa: E402
import sample_model as smp  # noqa: E402
import scores_model as sm  # noqa: E402
import ts_ref  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
TOKEN_BOUND = 1.1e-4  # section 15
BEAM_DELTA = 2e-4     # section 23: the beam chain's sums, and the margin above which a search is decisive


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def models(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    d = tmp_path_factory.mktemp("best_of")
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
def gold():
    return bm.load_golden()


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
    picked, sums, counts = eng.last_best_of()
    return ids, n, eng.last_scores(), eng.last_token_logprobs(ids.shape[1]), picked, sums, counts


def case_mel(mels, name, clips=None):
    mode, _, _, n_clips, _ = bm.CASES[name]
    clips = n_clips if clips is None else clips
    return np.ascontiguousarray(mels[mode][[b % mels[mode].shape[0] for b in range(clips)]])


def check(eng, got, g, name, clips):
    """The first `clips` clips of a case against its recorded reference."""
    mode, N, milli, _, P = bm.CASES[name]
    n0 = n0_of(mode)
    ids, n, sc, lp, picked, sums, counts = got
    info = eng.last_decode_info()
    assert ids.shape[0] == clips == picked.size == info.size
    exact = 0
    for c in range(clips):
        assert (info["temperature_milli"][c], info["attempts"][c], info["needs_fallback"][c]) == (milli, 1, 0)
        assert abs(sc["no_speech_prob"][c] - g["nosp"][c]) <= (TOKEN_BOUND + 2.0 ** -23) * g["nosp"][c]
        assert not sums[c, N:].any() and not counts[c, N:].any()
        if g["decisive"][c]:
            assert c not in bm.SET_ASIDE[name]
            assert picked[c] == g["picked"][c], (c, picked[c], sums[c], counts[c])
            for j in range(N):
                k = g["n_ids"][c, j] - n0
                assert counts[c, j] == k, (c, j)
                want = float(g["lps"][c, j, :k].sum())
                assert abs(sums[c, j] - want) <= TOKEN_BOUND * k + abs(want) * 2.0 ** -23, (c, j)
        elif picked[c] != g["picked"][c]:
            continue  # set aside, and the engine's averages fell the other way: another sample's row
        j = int(picked[c])
        k = int(g["compared"][c, j])
        assert [int(x) for x in ids[c, : n0 + k]] == [int(x) for x in g["ids"][c, j, : n0 + k]], c
        err = float(np.abs(lp[c, n0: n0 + k].astype(np.float64) - g["lps"][c, j, :k]).max()) if k else 0.0
        assert err <= TOKEN_BOUND, (c, err)
        if k < g["n_ids"][c, j] - n0:
            continue
        exact += 1
        assert n[c] == g["n_ids"][c, j] and sc["n_generated"][c] == k and counts[c, j] == k
        assert not lp[c, :n0].any() and not lp[c, n[c]:].any() and not ids[c, n[c]:].any()
        assert sc["sum_logprob"][c] == np.float32(sums[c, j])
        assert abs(sc["avg_logprob"][c] - sums[c, j] / k) <= abs(sums[c, j] / k) * 2.0 ** -23
    assert exact >= clips - len([c for c in bm.SET_ASIDE[name] if c < clips])


@pytest.mark.parametrize("name", ["ts-5x5-hot", "ts-2x5-cool", "plain-2x1-long"])
def test_best_of_equals_the_reference(pkg, models, mels, gold, name):
    """Eager, captured and replayed, without graphs, and (ts-5x5-hot) one clip alone."""
    mode, N, milli, clips, P = bm.CASES[name]
    eng = new_engine(pkg, models, mode, P, temperature=milli, seed=bm.SEEDS[name], best_of=N)
    assert eng.get_option("best_of") == N
    mel = case_mel(mels, name)
    first = decode(eng, mel)           # eager, then captured
    check(eng, first, gold[name], name, clips)
    again = decode(eng, mel)           # the segment graphs replayed: the same bits
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    if clips > 1:
        check(eng, decode(eng, mel[:1]), gold[name], name, 1)  # clip 0 alone keeps its index: the same reference
    eng.set_option("use_graphs", 0)
    eager = decode(eng, mel)
    for a, b in zip(first, eager):
        assert a.tobytes() == b.tobytes()
    eng.close()


def test_25_clips_fill_a_chain_and_26_run_two(pkg, models, mels, gold):
    """N = 5: 25 clips are the 125 rows of one chain, the 26th clip runs a second chain under its own clip index."""
    name = "ts-5x26-hot"
    mode, N, milli, clips, P = bm.CASES[name]
    eng = new_engine(pkg, models, mode, P, temperature=milli, seed=bm.SEEDS[name], best_of=N)
    mel = case_mel(mels, name)
    g26 = decode(eng, mel)
    check(eng, g26, gold[name], name, 26)
    g25 = decode(eng, mel[:25])
    check(eng, g25, gold[name], name, 25)
    # a clip's result depends on its own index alone: the same ids and picks in a chain of another size
    assert np.array_equal(g26[0][:25], g25[0]) and np.array_equal(g26[4][:25], g25[4])
    for a, b in zip(g26, decode(eng, mel)):  # replayed
        assert a.tobytes() == b.tobytes()
    eng.set_option("seed", smp.OTHER_SEED)  # the same graphs under another seed: other samples, the same twice
    other = decode(eng, mel[:5])
    assert not np.array_equal(other[0], g26[0][:5])
    for a, b in zip(other, decode(eng, mel[:5])):
        assert a.tobytes() == b.tobytes()
    eng.close()


def check_fallback(eng, g, mel):
    """Two calls (eager + captured, then replayed) against a recorded fall-back case: ids, decode info, scores, token
    log-probabilities, segments and the best-of record are the merged result's.  A clip kept at temperature 0 reports
    sample 0 and its own sum; where that attempt was the beam search (the case records the search's margin) the sums
    are within section 23's delta, elsewhere every token within section 15's bound."""
    n0 = len(sm.TS_PROMPT)
    for rnd in range(2):
        ids, n, sc, lp, picked, sums, counts = decode(eng, mel)
        info = eng.last_decode_info()
        assert eng.timings().decoder_steps > smp.P_SHORT  # summed over the attempts
        for b in range(mel.shape[0]):
            k = int(g["n_ids"][b, 0]) - n0
            beam = bool(np.isfinite(g["margin"][b]))  # kept from the beam search: the case records the search's margin
            assert not beam or g["margin"][b] > BEAM_DELTA  # (every recorded search is decisive)
            assert [int(x) for x in ids[b, : n[b]]] == [int(x) for x in g["ids"][b, 0, : g["n_ids"][b, 0]]], b
            assert (int(info["attempts"][b]), int(info["temperature_milli"][b]), int(info["needs_fallback"][b])) == \
                (int(g["attempts"][b]), int(g["milli"][b]), int(g["needs"][b])), b
            assert info["compression_ratio"][b].tobytes() == np.float32(g["ratio"][b]).tobytes()
            err = float(np.abs(lp[b, n0: n[b]].astype(np.float64) - g["lps"][b, 0, :k]).max())
            want_sum = float(g["lps"][b, 0, :k].sum())
            print(f"round {rnd} clip {b}: kept at {g['milli'][b]} beam {beam} lp error {err:.2e} "
                  f"sum error {abs(sc['sum_logprob'][b] - want_sum):.2e}")
            assert err <= (BEAM_DELTA if beam else TOKEN_BOUND) and not lp[b, n[b]:].any() and not lp[b, :n0].any()
            if beam:
                assert abs(float(sc["sum_logprob"][b]) - want_sum) < BEAM_DELTA and abs(sums[b, 0] - want_sum) < BEAM_DELTA
            assert sc["n_generated"][b] == k and g["same"][b, picked[b]] == 1  # the kept sample, or one with its very ids
            want_avg = want_sum / k
            assert abs(sc["avg_logprob"][b] - want_avg) <= (BEAM_DELTA if beam else TOKEN_BOUND) + abs(want_avg) * 2.0 ** -23
            assert abs(sc["no_speech_prob"][b] - g["nosp"][b]) <= (TOKEN_BOUND + 2.0 ** -23) * g["nosp"][b]
            assert np.array_equal(counts[b], g["all_count"][b]), b
            bound = BEAM_DELTA if beam else TOKEN_BOUND * np.maximum(counts[b], 1) + 1e-6
            assert (np.abs(sums[b] - g["all_sum"][b]) <= bound).all(), b
        segs = eng.last_segments()
        want = []
        for b in range(mel.shape[0]):
            want += ts_ref.segments([int(x) for x in g["ids"][b, 0, : g["n_ids"][b, 0]]], n0, sm.EOT, sm.BEG, clip=b)
        assert [tuple(int(x) for x in s) for s in segs] == want


def test_fallback_with_best_of_equals_the_reference_loop(pkg, models, mels, gold):
    """sample_model's fall-back fixture with 3 samples at the attempts above 0 and the greedy decode at 0."""
    g = gold["fallback"]
    eng = new_engine(pkg, models, "ts", smp.P_SHORT, temperature_fallback=1, best_of=bm.FB_N, **smp.FB)
    assert set(g["attempts"].tolist()) == {1, 2, 3} and (g["picked"] > 0).any()
    check_fallback(eng, g, mels["ts"])
    eng.close()


def beam_engine(pkg, models, **options):
    return new_engine(pkg, models, "ts", smp.P_SHORT, beam_size=bm.FB_K, full_beam=1, **options)


def test_fallback_beam_equals_the_reference_loop(pkg, models, mels, gold):
    """Option fallback_beam: the attempt at temperature 0 is the 4-hypothesis beam search over all clips, the attempts at
    0.5 and 1.0 keep one of 3 samples; clips are accepted from the beam and from a best-of attempt."""
    g = gold["fallback_beam"]
    assert ((g["milli"] == 0) & (g["needs"] == 0)).any() and ((g["milli"] > 0) & (g["needs"] == 0)).any()
    eng = beam_engine(pkg, models, fallback_beam=1, temperature_fallback=1, best_of=bm.FB_N, **bm.FB_BEAM)
    assert eng.get_option("fallback_beam") == 1
    check_fallback(eng, g, mels["ts"])
    with pytest.raises(pkg.WtError):
        eng.last_beam_scores()  # the merged result is no beam result: wt_last_scores and wt_last_decode_info describe it
    eng.set_option("use_graphs", 0)
    check_fallback(eng, g, mels["ts"])
    eng.close()


def test_fallback_beam_off_and_idle_are_the_parents_bytes(pkg, models, mels):
    """fallback_beam = 0 refuses a temperature beside the beam in section 23's words; at 1 a beam call without a
    temperature, and a call with beam_size = 1, are what they were; a fixed temperature > 0 is the sampling call of an
    engine without a beam; a fall-back whose thresholds never trigger keeps the beam search's result for every clip."""
    mel = np.ascontiguousarray(mels["ts"][:5])
    eng = beam_engine(pkg, models)
    assert eng.get_option("fallback_beam") == 0
    for bad in (-1, 2):
        with pytest.raises(pkg.WtError) as e:
            eng.set_option("fallback_beam", bad)
        assert status_of(e) == INVALID
    beam = eng.encdec_tokens_full(mel) + eng.last_beam_scores() + (eng.last_scores(), eng.last_token_logprobs(smp.P_SHORT + 1))
    for key, on in (("temperature", 500), ("temperature_fallback", 1)):
        eng.set_option(key, on)
        with pytest.raises(pkg.WtError) as e:
            eng.encdec_tokens_full(mel)
        assert status_of(e) == UNSUPPORTED
        assert str(e.value).endswith("full-length beam search (full_beam): not with a temperature or the temperature fall-back")
        eng.set_option(key, 0)
    eng.set_option("fallback_beam", 1)
    same = eng.encdec_tokens_full(mel) + eng.last_beam_scores() + (eng.last_scores(), eng.last_token_logprobs(smp.P_SHORT + 1))
    for a, b in zip(beam, same):
        assert a.tobytes() == b.tobytes()
    # a fall-back that accepts everything at temperature 0: the beam search's ids and scores for every clip
    for k, v in (("temperature_fallback", 1), ("compression_ratio_threshold", 0), ("logprob_threshold", -1000000)):
        eng.set_option(k, v)
    kept = eng.encdec_tokens_full(mel) + (eng.last_scores(), eng.last_token_logprobs(smp.P_SHORT + 1))
    assert kept[0].tobytes() == beam[0].tobytes() and kept[1].tobytes() == beam[1].tobytes()
    assert kept[2].tobytes() == beam[4].tobytes() and kept[3].tobytes() == beam[5].tobytes()
    assert (eng.last_decode_info()["attempts"] == 1).all() and (eng.last_decode_info()["temperature_milli"] == 0).all()
    # a fixed temperature above 0 ignores the beam: the sampling call of an engine that has none
    eng.set_option("temperature_fallback", 0)
    eng.set_option("temperature", 1000)
    eng.set_option("seed", smp.SEED)
    eng.set_option("best_of", 2)
    sampled = decode(eng, mel)
    plain = new_engine(pkg, models, "ts", smp.P_SHORT, temperature=1000, seed=smp.SEED, best_of=2, fallback_beam=1)
    for a, b in zip(sampled, decode(plain, mel)):  # (fallback_beam without a beam means nothing)
        assert a.tobytes() == b.tobytes()
    plain.close()
    eng.close()


def test_fallback_beam_refusals(pkg, models, mels):
    """With fallback_beam = 1 the beam chain's scope holds: WT_ERR_UNSUPPORTED with a text, and the same call works
    once the option is taken back."""
    mel = np.ascontiguousarray(mels["ts"][:2])
    eng = beam_engine(pkg, models, fallback_beam=1, temperature_fallback=1, best_of=2, **bm.FB_BEAM)
    want = eng.encdec_tokens_full(mel)

    def refused(fn, undo):
        with pytest.raises(pkg.WtError) as e:
            fn()
        assert status_of(e) == UNSUPPORTED and len(str(e.value).split(":", 1)[1].strip()) > 0, str(e.value)
        undo()
        got = eng.encdec_tokens_full(mel)  # the engine stays usable: the same result again
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])

    call = lambda: eng.encdec_tokens_full(mel)  # noqa: E731
    for key, on in (("seek", 1), ("word_timestamps", 1), ("stop_at_eot", 0), ("cross_absorb", 0)):
        off = eng.get_option(key)
        eng.set_option(key, on)
        refused(call, lambda: eng.set_option(key, off))
    eng.set_context([5, 6, 7])
    refused(call, lambda: eng.set_context([]))
    eng.set_contexts([[5, 6], [7]])
    refused(call, lambda: eng.set_contexts([]))
    rng = np.random.default_rng(1)
    pcm = (0.1 * rng.standard_normal(eng.pcm_len)).astype(np.float32)
    refused(lambda: eng.transcribe_long_batch([pcm, pcm]), lambda: None)
    eng.close()
    # a default transcription on a fresh engine of the same files
    eng = pkg.Engine(models["ts"][0], models["ts"][1], True)
    ids, n = eng.encdec_tokens_batch(mel)
    assert ids.shape[0] == 2 and (n > 0).all()
    eng.close()


def test_two_windows_of_long_audio(pkg, models):
    """wt_transcribe_long_pcm with fixed windows: window w is clip w of the counter, as the token call on the same
    log-mel decodes it; wt_last_best_of has one entry per window."""
    eng = new_engine(pkg, models, "ts", smp.P_SHORT, temperature=1000, seed=smp.SEED, best_of=2)
    rng = np.random.default_rng(42)
    pcm = (0.1 * rng.standard_normal((2, eng.pcm_len))).astype(np.float32)
    mel = eng.logmel_batch(pcm)
    ids, n = eng.encdec_tokens_full(mel)
    record = eng.last_best_of()
    lines = eng.transcribe_long(pcm.reshape(-1)).split("\n")
    assert lines == [eng.decode_text(ids[b, : n[b]]) for b in range(2)]
    for a, b in zip(record, eng.last_best_of()):
        assert a.tobytes() == b.tobytes() and a.shape[0] == 2
    alone = eng.transcribe(pcm[1])  # window 1 as the only clip of a call: clip index 0, another sample
    ids1, n1 = eng.encdec_tokens_full(mel[1:2])
    assert alone == eng.decode_text(ids1[0, : n1[0]]) and eng.last_best_of()[0].size == 1
    eng.close()


def test_best_of_one_and_zero_temperature_are_the_parents_bytes(pkg, models, mels):
    """best_of = 1 is the sampling decode as it was; best_of = 5 at temperature 0 without fall-back is the greedy decode
    and leaves no best-of record; with fall-back whose thresholds never trigger it is the greedy decode too."""
    mel = np.ascontiguousarray(mels["ts"][:5])
    eng = new_engine(pkg, models, "ts", smp.P_SHORT, temperature=1000, seed=smp.SEED)
    assert eng.get_option("best_of") == 1
    base = eng.encdec_tokens_full(mel) + (eng.last_scores(), eng.last_token_logprobs(smp.P_SHORT + 1))
    eng.set_option("best_of", 1)
    same = eng.encdec_tokens_full(mel) + (eng.last_scores(), eng.last_token_logprobs(smp.P_SHORT + 1))
    for a, b in zip(base, same):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(pkg.WtError) as e:
        eng.last_best_of()
    assert status_of(e) == INVALID
    eng.set_option("temperature", 0)
    greedy = eng.encdec_tokens_full(mel) + (eng.last_scores(),)
    eng.set_option("best_of", 5)
    still = eng.encdec_tokens_full(mel) + (eng.last_scores(),)
    for a, b in zip(greedy, still):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(pkg.WtError) as e:
        eng.last_best_of()
    assert status_of(e) == INVALID
    for k, v in (("temperature_fallback", 1), ("compression_ratio_threshold", 0), ("logprob_threshold", -1000000)):
        eng.set_option(k, v)
    kept = eng.encdec_tokens_full(mel)
    assert np.array_equal(kept[0], greedy[0]) and np.array_equal(kept[1], greedy[1])
    assert (eng.last_decode_info()["attempts"] == 1).all()
    with pytest.raises(pkg.WtError):
        eng.last_best_of()  # every clip was kept at temperature 0
    eng.close()


def test_option_range_and_refusals(pkg, models, mels):
    three = np.ascontiguousarray(mels["plain"][:3])
    eng = pkg.Engine(models["plain"][0], models["plain"][1], True)
    parent_ids, parent_n = eng.encdec_tokens_batch(three)
    with pytest.raises(pkg.WtError) as e:
        eng.last_best_of()  # before any such decode
    assert status_of(e) == INVALID
    for bad in (0, 9, -1):
        with pytest.raises(pkg.WtError) as e:
            eng.set_option("best_of", bad)
        assert status_of(e) == INVALID
    assert eng.get_option("best_of") == 1
    for ok in (8, 2):
        eng.set_option("best_of", ok)
        assert eng.get_option("best_of") == ok
    ids, n = eng.encdec_tokens_batch(three)  # without a temperature the option changes nothing, anywhere
    assert np.array_equal(ids, parent_ids) and np.array_equal(n, parent_n)

    def refused(fn, undo):
        with pytest.raises(pkg.WtError) as e:
            fn()
        assert status_of(e) == UNSUPPORTED, str(e.value)
        assert "best_of" in str(e.value) and len(str(e.value).split(":", 1)[1].strip()) > 0
        undo()
        keep = {k: eng.get_option(k) for k in ("max_positions", "temperature", "best_of")}
        for k in keep:
            eng.set_option(k, {"max_positions": 0, "temperature": 0, "best_of": 1}[k])
        ids, n = eng.encdec_tokens_batch(three)  # the engine stays usable: a default call gives the parent's ids
        assert np.array_equal(ids, parent_ids) and np.array_equal(n, parent_n)
        for k, v in keep.items():
            eng.set_option(k, v)

    eng.set_option("max_positions", sm.P_PLAIN)
    eng.set_option("temperature", 600)
    call = lambda: eng.encdec_tokens_full(three)  # noqa: E731
    eng.set_context(np.array([5, 6, 7], np.int64))
    refused(call, lambda: eng.set_context([]))
    eng.set_option("stop_at_eot", 0)
    refused(call, lambda: eng.set_option("stop_at_eot", 1))
    eng.set_option("cross_absorb", 0)
    refused(call, lambda: eng.set_option("cross_absorb", 1))
    pcm = np.zeros(1600, np.float32)
    refused(lambda: eng.transcribe_long_batch([pcm]), lambda: None)
    eng.encdec_tokens_full(three)  # everything restored: a best-of call works, with or without scores
    assert eng.last_best_of()[0].size == 3
    eng.close()
    # seek and word_timestamps live on the timestamp model
    eng = new_engine(pkg, models, "ts", smp.P_SHORT, temperature=600, best_of=2)
    mel = np.ascontiguousarray(mels["ts"][:2])
    for key in ("seek", "word_timestamps"):
        eng.set_option(key, 1)
        with pytest.raises(pkg.WtError) as e:
            eng.encdec_tokens_full(mel)
        assert status_of(e) == UNSUPPORTED and "best_of" in str(e.value), key
        eng.set_option(key, 0)
        eng.encdec_tokens_full(mel)
        assert eng.last_best_of()[0].size == 2
    eng.close()


def test_the_cli_sets_fallback_beam_itself(pkg, models, tmp_path):
    """encdec --beam K --max-positions P --fallback sets fallback_beam as --beam sets full_beam: the text is the
    library call's under the same options."""
    import struct
    import subprocess
    eng = beam_engine(pkg, models, fallback_beam=1, temperature_fallback=1, best_of=bm.FB_N, seed=smp.SEED)
    rng = np.random.default_rng(7)
    pcm16 = np.clip(np.round(0.1 * rng.standard_normal(eng.pcm_len) * 32767), -32768, 32767).astype("<i2")
    wav = tmp_path / "noise.wav"
    wav.write_bytes(b"RIFF" + struct.pack("<I", 36 + pcm16.nbytes) + b"WAVEfmt " +
                    struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" + struct.pack("<I", pcm16.nbytes) +
                    pcm16.tobytes())
    eng.transcribe(str(wav))
    segs, texts = eng.last_segments(with_text=True)
    eng.close()
    exe = os.path.join(ROOT, "whisper.tflite_amd", "bin", "encdec")
    r = subprocess.run([exe, "--model-prefix", models["ts"][0], "--vocab", models["ts"][1], "--input", str(wav), "--beam",
                        str(bm.FB_K), "--max-positions", str(smp.P_SHORT), "--timestamps", "--scores", "--fallback",
                        "--best-of", str(bm.FB_N), "--seed", str(smp.SEED)], capture_output=True, text=True, errors="replace",
                       timeout=120)
    assert r.returncode == 0, r.stderr
    stamp = lambda ms: "%02d:%02d.%03d" % (ms // 60000, ms // 1000 % 60, ms % 1000)  # noqa: E731
    lines = [ln.rsplit(" (avg_logprob=", 1)[0] for ln in r.stdout.splitlines() if ln.startswith("[")]
    assert len(texts) >= 1
    assert lines == [("[%s --> %s] %s" % (stamp(int(s[1])), stamp(int(s[2])), t.decode("utf-8", errors="replace")))
                     for s, t in zip(segs, texts)]
    assert "window 0: temperature=" in r.stdout
