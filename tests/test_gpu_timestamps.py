"""Timestamp decoding (options timestamps + max_positions) on the GPU against tests/ts_ref.py over
the CPU oracle, on the model of tests/ts_model.py (tests/test_ts_reference.py pins what the reference gives on it).
Without the feature set_option("timestamps", 1) fails and so does every test here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ts_model as tm  # noqa: E402
import ts_ref  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
N0 = len(tm.PROMPT)


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def model(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("ts") / "micro-ts")
    tm.write_model(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def mel():
    m = tm.mels()
    m.setflags(write=False)
    return m


@pytest.fixture(scope="module")
def ref(orc, model, mel):
    """ts_ref over the oracle at P_LONG, computed once; P_SHORT is its cut (test_ts_reference.py checks that)."""
    m = orc.Model(model[0] + ".wtw")
    rows = tm.reference_rows(m, mel, tm.P_LONG)
    m.close()
    return {tm.P_LONG: rows, tm.P_SHORT: tm.cut_rows(rows, tm.P_SHORT)}


def new_engine(pkg, model, positions=tm.P_LONG, **kw):
    eng = pkg.Engine(model[0], model[1], True, **kw)
    eng.set_option("max_positions", positions)
    eng.set_option("timestamps", 1)
    return eng


@pytest.fixture(scope="module")
def eng(pkg, model):
    e = new_engine(pkg, model)
    info = e.vocab_info()
    assert (info["eot"], info["beg"]) == (tm.EOT, tm.BEG) and e.dims.n_text_ctx == tm.N_TEXT_CTX
    yield e
    e.close()


def rows_of(ids, n):
    return [[int(x) for x in ids[b, : n[b]]] for b in range(ids.shape[0])]


def check(got_rows, ref_rows, clips=None):
    """Ids and counts equal the reference on every decisive clip; an indecisive clip up to its first indecisive step."""
    clips = range(len(ref_rows)) if clips is None else clips
    assert len(got_rows) == len(clips)
    for got, b in zip(got_rows, clips):
        want, infos = ref_rows[b]
        s = ts_ref.first_indecisive(infos, tm.MARGIN)
        if s is None:
            assert got == want, (b, got, want)
        else:
            assert got[: N0 + s] == want[: N0 + s], (b, s)


@pytest.mark.parametrize("positions", [tm.P_LONG, tm.P_SHORT])
def test_ids_and_counts_equal_the_reference(eng, mel, ref, positions):
    eng.set_option("max_positions", positions)
    ids, n = eng.encdec_tokens_full(mel)
    assert ids.shape == (tm.CLIPS, positions + 1)
    for b in range(tm.CLIPS):
        assert not ids[b, n[b]:].any()
        assert list(ids[b, :N0]) == tm.PROMPT  # the default prompt without <|notimestamps|>
    check(rows_of(ids, n), ref[positions])
    again = eng.encdec_tokens_full(mel)  # the segment graphs replayed
    assert np.array_equal(again[0], ids) and np.array_equal(again[1], n)
    eng.set_option("max_positions", tm.P_LONG)


def test_batch_sizes_cross_attention_forms_and_eager(pkg, model, mel, ref):
    """1, 5 and 64 rows; 64 clips take the absorbed cross-attention (and the cached one with cross_absorb = 0); with
    and without hipGraphs."""
    e = new_engine(pkg, model)
    want = ref[tm.P_LONG]
    pick = [b % tm.CLIPS for b in range(64)]
    mel64 = np.ascontiguousarray(mel[pick])
    assert e.get_option("cross_absorb_active") == 1
    r64 = rows_of(*e.encdec_tokens_full(mel64))
    check(r64, want, pick)
    check(rows_of(*e.encdec_tokens_full(np.ascontiguousarray(mel[:5]))), want, range(5))
    check(rows_of(*e.encdec_tokens_full(np.ascontiguousarray(mel[3:4]))), want, [3])
    assert rows_of(*e.encdec_tokens_full(mel64)) == r64  # replay
    e.set_option("cross_absorb", 0)
    check(rows_of(*e.encdec_tokens_full(mel64)), want, pick)
    e.set_option("use_graphs", 0)
    check(rows_of(*e.encdec_tokens_full(mel64)), want, pick)
    check(rows_of(*e.encdec_tokens_full(np.ascontiguousarray(mel[:5]))), want, range(5))
    e.set_option("cross_absorb", 1)
    assert rows_of(*e.encdec_tokens_full(mel64)) == r64
    e.close()


def test_max_initial_timestamp(eng, mel):
    one = np.ascontiguousarray(mel[:2])
    eng.set_option("max_initial_timestamp", 5)
    assert eng.get_option("max_initial_timestamp") == 5
    ids, _ = eng.encdec_tokens_full(one)
    assert ((ids[:, N0] >= tm.BEG) & (ids[:, N0] <= tm.BEG + 5)).all()
    eng.set_option("max_initial_timestamp", -1)
    ids, _ = eng.encdec_tokens_full(one)
    assert (ids[:, N0] >= tm.BEG).all()
    for bad in (-2, 1501):
        with pytest.raises(Exception) as e:
            eng.set_option("max_initial_timestamp", bad)
        assert status_of(e) == INVALID
    eng.set_option("max_initial_timestamp", 50)


def seg_tuples(segs):
    return [tuple(int(x) for x in s) for s in segs]


def test_last_segments_equal_the_python_parse(eng, mel):
    ids, n = eng.encdec_tokens_full(mel)
    want = []
    for b in range(tm.CLIPS):
        want += ts_ref.segments(ids[b, : n[b]], N0, tm.EOT, tm.BEG, clip=b)
    segs, texts = eng.last_segments(with_text=True)
    assert seg_tuples(segs) == want and len(want) >= tm.CLIPS
    assert any(s[5] for s in want) and any(not s[5] for s in want)
    for s, t in zip(want, texts):
        assert t.decode("utf-8", errors="replace") == eng.decode_text(ids[s[0], s[3]: s[3] + s[4]])


def test_text_entry_points_and_the_long_audio_offset(eng):
    rng = np.random.default_rng(42)
    pcm = (0.1 * rng.standard_normal((2, eng.pcm_len))).astype(np.float32)
    ids, n = eng.encdec_tokens_full(eng.logmel_batch(pcm))
    texts = [eng.transcribe(pcm[b]) for b in range(2)]
    for b in range(2):
        assert texts[b] == eng.decode_text(ids[b, : n[b]])  # timestamp ids print as the vocabulary's token strings
    assert seg_tuples(eng.last_segments()) == ts_ref.segments(ids[1, : n[1]], N0, tm.EOT, tm.BEG)
    assert eng.transcribe_long(pcm.reshape(-1)) == "\n".join(texts)
    want = []
    for w in range(2):  # two windows: clip = the window, 30 000 ms x the window added to both times
        for (_, t0, t1, i0, cnt, op) in ts_ref.segments(ids[w, : n[w]], N0, tm.EOT, tm.BEG):
            want.append((w, t0 + 30000 * w, t1 + 30000 * w, i0, cnt, op))
    assert seg_tuples(eng.last_segments()) == want and any(s[0] == 1 for s in want)


def test_option_off_changes_nothing(pkg, model, mel):
    three = np.ascontiguousarray(mel[:3])
    plain = pkg.Engine(model[0], model[1], True)  # never had the option
    plain.set_option("max_positions", tm.P_LONG)
    want_full = plain.encdec_tokens_full(three)
    plain.set_option("max_positions", 0)
    want31 = plain.encdec_tokens_batch(three)
    with pytest.raises(pkg.WtError) as e:
        plain.last_segments()
    assert status_of(e) == INVALID
    plain.close()
    eng = new_engine(pkg, model)
    with_ts = eng.encdec_tokens_full(three)
    assert not np.array_equal(with_ts[0], want_full[0])
    assert eng.last_segments().size > 0
    eng.set_option("timestamps", 0)
    off = eng.encdec_tokens_full(three)  # off again: the ids of an engine that never had it
    assert np.array_equal(off[0], want_full[0]) and np.array_equal(off[1], want_full[1])
    with pytest.raises(pkg.WtError):
        eng.last_segments()  # the last decode ran without timestamps
    eng.set_option("timestamps", 1)
    eng.encdec_tokens_full(three)
    eng.set_option("timestamps", 0)
    eng.set_option("max_positions", 0)
    got31 = eng.encdec_tokens_batch(three)  # after a timestamp call an ordinary 31-position call gives its old ids
    assert np.array_equal(got31[0], want31[0]) and np.array_equal(got31[1], want31[1])
    eng.close()


def test_refusals(pkg, model, mel, assets):
    import ctypes
    from conftest import DevBuf
    three = np.ascontiguousarray(mel[:3])
    eng = pkg.Engine(model[0], model[1], True)
    parent_ids, parent_n = eng.encdec_tokens_batch(three)
    keys = ("timestamps", "max_positions", "beam_size", "bf16", "language")

    def refused(fn, code=UNSUPPORTED):
        with pytest.raises(pkg.WtError) as e:
            fn()
        assert status_of(e) == code, str(e.value)
        assert len(str(e.value).split(":", 1)[1].strip()) > 0  # a wt_last_error text
        keep = {k: eng.get_option(k) for k in keys}  # the engine stays usable: a default call gives the parent's ids
        for k, v in (("timestamps", 0), ("max_positions", 0), ("beam_size", 1), ("bf16", 0), ("language", 2)):
            eng.set_option(k, v)
        eng.set_forced_ids(None)
        ids, n = eng.encdec_tokens_batch(three)
        assert np.array_equal(ids, parent_ids) and np.array_equal(n, parent_n)
        for k in ("language", "bf16", "beam_size", "max_positions", "timestamps"):
            eng.set_option(k, keep[k])

    for bad in (-1, 2):
        with pytest.raises(pkg.WtError) as e:
            eng.set_option("timestamps", bad)
        assert status_of(e) == INVALID
    eng.set_option("timestamps", 1)
    assert eng.get_option("timestamps") == 1 and eng.get_option("max_initial_timestamp") == 50
    dev = DevBuf(three)
    pcm = np.zeros(1600, np.float32)
    # without max_positions: every decode call
    refused(lambda: eng.encdec_tokens_batch(three))
    refused(lambda: eng.encdec_tokens_batch_dev(dev.data_ptr(), 3))
    refused(lambda: eng.encdec_tokens_full(three, ids_stride=tm.P_LONG + 1))
    refused(lambda: eng.transcribe(pcm))
    refused(lambda: eng.transcribe_long(pcm))
    refused(lambda: eng.pipeline_submit_dev(dev.data_ptr(), 3))
    eng._submitted = []
    assert eng.get_option("in_flight") == 0
    # with it: whatever max_positions refuses
    eng.set_option("max_positions", tm.P_LONG)
    refused(lambda: eng.encdec_tokens_batch(three))                # the [B][32] calls
    refused(lambda: eng.transcribe_tokens_batch_dev(dev.data_ptr(), 3))
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
    refused(lambda: eng.transcribe(pcm))
    eng.set_option("language", 2)
    forced = np.zeros((3, 32), np.int64)
    forced[:, :N0] = tm.PROMPT
    assert pkg.lib().wt_dbg_set_forced_ids(eng.handle, forced.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 3) == 0
    refused(lambda: eng.encdec_tokens_full(three))  # (refused() switches the tap off again)
    dev.free()
    ids, n = eng.encdec_tokens_full(three)  # everything restored: a timestamp call works
    assert (ids[:, N0] >= tm.BEG).all()
    eng.close()
    # a vocabulary without timestamp ids: the option itself is refused
    prefix, vocab = assets("micro")
    small = pkg.Engine(prefix, vocab, True)
    with pytest.raises(pkg.WtError) as e:
        small.set_option("timestamps", 1)
    assert status_of(e) == UNSUPPORTED and small.get_option("timestamps") == 0
    small.close()


def test_caller_prompt_and_monolith_prompt(pkg, model, mel):
    two = np.ascontiguousarray(mel[:2])
    eng = new_engine(pkg, model, 64)
    eng.set_prompt([50258, 50259, 50359, 50363])  # used as given, <|notimestamps|> included
    ids, n = eng.encdec_tokens_full(two)
    assert list(ids[0, :4]) == [50258, 50259, 50359, 50363] and (ids[:, 4] >= tm.BEG).all()
    eng.close()
    mono = new_engine(pkg, model, 64, engine_type=pkg.EngineType.Monolith)
    ids, n = mono.encdec_tokens_full(two)
    sot = mono.vocab_info()["sot"]
    assert list(ids[0, :3]) == [sot, 50259, mono.vocab_info()["transcribe"]] and (ids[:, 3] >= tm.BEG).all()
    mono.close()
