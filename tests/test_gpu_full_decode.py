"""Full-length greedy decoding (option max_positions) on the GPU against the CPU oracle's
decode_greedy at the same max_positions, on the 160-position models of tests/full_model.py (test_full_reference.py pins
what the oracle gives on them).  Without the feature the option and the entry points do not exist and every test here
fails."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import full_model as fm  # noqa: E402

pytestmark = pytest.mark.gpu

P = fm.N_TEXT_CTX
UNSUPPORTED, INVALID, BUFFER = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG", "WT_ERR_BUFFER"


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def dense(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("full") / "micro-full-dense")
    fm.write_dense(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def rich(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("full") / "micro-full-rich")
    fm.write_eot_rich(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def rich_mel():
    mel = fm.mels(fm.RICH_CLIPS, (80, 200), fm.RICH_SEED)
    mel.setflags(write=False)
    return mel


@pytest.fixture(scope="module")
def rich_ref(orc, rich, rich_mel):
    """The oracle's rows on the EOT-rich model at P = 160 and P = 40, computed once."""
    model = orc.Model(rich[0] + ".wtw")
    ref = {p: fm.oracle_rows(model, rich_mel, fm.RICH_PROMPT, p, fm.EOT) for p in (P, 40)}
    model.close()
    for rows in ref.values():  # exact comparison below: no step of these clips is anywhere near a tie
        assert min(float(m.min()) for _, m in rows) > 10 * fm.MARGIN
    return ref


@pytest.fixture(scope="module")
def rich_eng(pkg, rich):
    eng = pkg.Engine(rich[0], rich[1], True)
    assert eng.vocab_info()["eot"] == fm.EOT and eng.dims.n_text_ctx == P
    yield eng
    eng.close()


def rows_of(ids, n):
    return [[int(x) for x in ids[b, : n[b]]] for b in range(ids.shape[0])]


def check_padding(ids, n):
    for b in range(ids.shape[0]):
        assert not ids[b, n[b]:].any()


def compare_with_margin_rule(got_rows, ref_rows, n_prompt, max_aside):
    """The decisive-margin rule: a clip whose ids first differ at a step where the oracle's top-two margin is below
    fm.MARGIN is set aside from that step on; any other difference fails.  Returns the clips set aside."""
    aside = []
    for b, (got, (want, margins)) in enumerate(zip(got_rows, ref_rows)):
        if got == want:
            continue
        i = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
        assert i >= n_prompt, (b, i)
        step = i - n_prompt
        assert step < len(margins) and margins[step] < fm.MARGIN, (b, i, got[i - 2:i + 2], want[i - 2:i + 2], float(margins[min(step, len(margins) - 1)]))
        aside.append((b, i))
    assert len(aside) <= max_aside, aside
    return aside


def test_dense_model_matches_greedy_and_the_oracle(pkg, orc, dense):
    prefix, vocab = dense
    eng = pkg.Engine(prefix, vocab, True)
    eng.set_prompt(fm.DENSE_PROMPT)
    mel = fm.dense_mels(eng.mel_shape)
    assert eng.get_option("max_positions") == 0
    ids31, n31 = eng.encdec_tokens_batch(mel)  # the option off: the max_tokens path, 31 ids
    assert list(n31) == [31] * 6
    eng.set_option("max_positions", P)
    assert eng.get_option("max_positions") == P
    ids, n = eng.encdec_tokens_full(mel)
    assert ids.shape == (6, P + 1) and list(n) == [P + 1] * 6  # the micro vocabulary has no EOT
    # the same kernels on a larger cache: exact
    assert np.array_equal(ids[:, :31], ids31[:, :31])
    model = orc.Model(prefix + ".wtw")
    ref = fm.oracle_rows(model, mel, fm.DENSE_PROMPT, P, eng.vocab_info()["eot"])
    model.close()
    aside = compare_with_margin_rule(rows_of(ids, n), ref, len(fm.DENSE_PROMPT), max_aside=1)
    print("dense clips set aside:", aside)
    eng.set_option("max_positions", 0)
    again, n_again = eng.encdec_tokens_batch(mel)
    assert np.array_equal(again, ids31) and np.array_equal(n_again, n31)
    eng.close()


@pytest.mark.parametrize("positions", [P, 40])
def test_eot_rich_ids_and_counts_equal_the_oracle(rich_eng, rich_mel, rich_ref, positions):
    eng = rich_eng
    eng.set_option("max_positions", positions)
    ids, n = eng.encdec_tokens_full(rich_mel)
    check_padding(ids, n)
    want = [r[0] for r in rich_ref[positions]]
    assert [int(x) for x in n] == [len(w) for w in want]
    assert rows_of(ids, n) == want
    assert max(len(w) for w in want) == positions + 1  # a clip runs to the cap


def test_fc2_ksplit_1_ids_and_counts_equal_the_oracle(pkg, rich, rich_mel, rich_ref):
    """The chains share one decoder pass: full-length decoding with fc2 unsplit (fc2_ksplit = 1, x handed from layer to
    layer and to the logits GEMM whole instead of as two halves), 2 clips at P = 40: one ends early, one runs to the cap
    (positions past 32, the second segment)."""
    eng = pkg.Engine(rich[0], rich[1], True)
    eng.set_option("fc2_ksplit", 1)
    eng.set_option("max_positions", 40)
    ids, n = eng.encdec_tokens_full(np.ascontiguousarray(rich_mel[[0, 1]]))
    check_padding(ids, n)
    want = [rich_ref[40][b][0] for b in (0, 1)]
    assert [int(x) for x in n] == [len(w) for w in want]
    assert rows_of(ids, n) == want
    assert len(want[0]) < 32 and len(want[1]) == 41
    eng.close()


def test_segment_stop(rich_eng, rich_mel, rich_ref):
    """A chain whose clips all finished inside the first 32 positions ends there; a mixed one runs on."""
    eng = rich_eng
    eng.set_option("max_positions", P)
    fin = [fm.finish_index(r[0]) for r in rich_ref[P]]
    early = [b for b, f in enumerate(fin) if f is not None and f < 32]
    assert len(early) >= 2
    ids, n = eng.encdec_tokens_full(np.ascontiguousarray(rich_mel[early]))
    assert rows_of(ids, n) == [rich_ref[P][b][0] for b in early]
    steps_early = eng.timings().decoder_steps
    assert 0 < steps_early <= 32, steps_early
    eng.encdec_tokens_full(rich_mel)
    steps_mixed = eng.timings().decoder_steps
    assert steps_mixed == P - len(fm.RICH_PROMPT) + 1, steps_mixed  # a clip runs to the cap: every step
    # clips that finish in the middle: the chain ends with the segment of the last EOT
    mid = [b for b, f in enumerate(fin) if f is not None and 33 <= f < 96]
    assert mid
    ids, n = eng.encdec_tokens_full(np.ascontiguousarray(rich_mel[mid]))
    assert rows_of(ids, n) == [rich_ref[P][b][0] for b in mid]
    last = max(fin[b] for b in mid)
    # the EOT at row index `last` is chosen at position last - 1; the chain ends with that position's segment
    assert eng.timings().decoder_steps == 32 * ((last - 1) // 32 + 1) - len(fm.RICH_PROMPT) + 1


def test_graphs_replay_and_eager_agree(pkg, rich, rich_mel, rich_ref):
    eng = pkg.Engine(rich[0], rich[1], True)
    eng.set_option("max_positions", P)
    want = [r[0] for r in rich_ref[P]]
    two = np.ascontiguousarray(rich_mel[[4, 5]])
    assert rows_of(*eng.encdec_tokens_full(two)) == [want[4], want[5]]  # a 2-clip cache and its graphs ...
    assert rows_of(*eng.encdec_tokens_full(two)) == [want[4], want[5]]  # ... replayed
    a = eng.encdec_tokens_full(rich_mel)  # 12 clips: the cache grows, the 2-clip graphs go with it; eager, then captured
    b = eng.encdec_tokens_full(rich_mel)  # replayed
    short = eng.encdec_tokens_full(two)  # a shorter chain after a longer one, captured again on the larger cache
    assert rows_of(*short) == [want[4], want[5]]
    c = eng.encdec_tokens_full(rich_mel)
    eng.set_option("use_graphs", 0)
    e = eng.encdec_tokens_full(rich_mel)
    assert rows_of(*a) == want
    for x in (b, c, e):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])
    eng.close()


def test_batch_sizes_and_cross_attention_forms_agree(pkg, rich, rich_mel, rich_ref):
    """1, 5 and 64 rows, clip by clip: small synchronous calls take the cached cross-attention, 64 clips the absorbed
    one (and the cached one with cross_absorb = 0)."""
    eng = pkg.Engine(rich[0], rich[1], True)
    eng.set_option("max_positions", P)
    want = [r[0] for r in rich_ref[P]]
    mel64 = np.ascontiguousarray(rich_mel[[b % fm.RICH_CLIPS for b in range(64)]])
    assert eng.get_option("cross_absorb_active") == 1
    r64 = rows_of(*eng.encdec_tokens_full(mel64))
    assert r64 == [want[b % fm.RICH_CLIPS] for b in range(64)]
    r5 = rows_of(*eng.encdec_tokens_full(np.ascontiguousarray(rich_mel[:5])))
    r1 = rows_of(*eng.encdec_tokens_full(np.ascontiguousarray(rich_mel[3:4])))
    assert r5 == want[:5] and r1 == [want[3]]
    eng.set_option("cross_absorb", 0)
    assert rows_of(*eng.encdec_tokens_full(mel64)) == r64
    with pytest.raises(pkg.WtError) as e:  # more than 64 clips stay refused
        eng.encdec_tokens_full(np.zeros((65,) + tuple(eng.mel_shape), np.float32))
    assert status_of(e) == INVALID
    eng.close()


def test_text_entry_points_honour_the_option(rich_eng):
    eng = rich_eng
    eng.set_option("max_positions", P)
    rng = np.random.default_rng(42)
    pcm = (0.1 * rng.standard_normal((2, eng.pcm_len))).astype(np.float32)
    ids, n = eng.encdec_tokens_full(eng.logmel_batch(pcm))
    texts = [eng.transcribe(pcm[b]) for b in range(2)]
    for b in range(2):
        assert texts[b] == eng.decode_text(ids[b, : n[b]])
    assert eng.transcribe_long(pcm.reshape(-1)) == "\n".join(texts)
    from conftest import DevBuf
    dev = DevBuf(pcm)
    ids2, n2 = eng.transcribe_tokens_full_dev(dev.data_ptr(), 2)
    dev.free()
    assert np.array_equal(ids2, ids) and np.array_equal(n2, n)
    eng.set_option("max_positions", 0)
    short = eng.transcribe(pcm[0])
    ids31, n31 = eng.encdec_tokens_batch(eng.logmel_batch(pcm[:1]))
    assert short == eng.decode_text(ids31[0, : n31[0]])


def test_status_codes_and_scope_cuts(pkg, rich, rich_mel):
    import ctypes
    from conftest import DevBuf
    eng = pkg.Engine(rich[0], rich[1], True)
    mel = np.ascontiguousarray(rich_mel[:3])
    parent_ids, parent_n = eng.encdec_tokens_batch(mel)

    def refused(code, fn):
        with pytest.raises(pkg.WtError) as e:
            fn()
        assert status_of(e) == code, str(e.value)
        assert len(str(e.value).split(":", 1)[1].strip()) > 0  # a wt_last_error text
        # the engine stays usable: a default greedy call still returns the parent's ids
        keep = eng.get_option("max_positions")
        others = {k: eng.get_option(k) for k in ("beam_size", "bf16", "language")}
        eng.set_option("max_positions", 0)
        for k, v in (("beam_size", 1), ("bf16", 0), ("language", 2)):
            eng.set_option(k, v)
        eng.set_forced_ids(None)
        ids, n = eng.encdec_tokens_batch(mel)
        assert np.array_equal(ids, parent_ids) and np.array_equal(n, parent_n)
        for k, v in others.items():
            eng.set_option(k, v)
        eng.set_option("max_positions", keep)

    # the option's range
    for bad in (-1, 1, 31, P + 1, 448):
        with pytest.raises(pkg.WtError) as e:
            eng.set_option("max_positions", bad)
        assert status_of(e) == INVALID
    for ok in (32, P, 0):
        eng.set_option("max_positions", ok)
        assert eng.get_option("max_positions") == ok
    # the full-length entry points need the option
    refused(INVALID, lambda: eng.encdec_tokens_full(mel, ids_stride=P + 1))
    eng.set_option("max_positions", P)
    refused(BUFFER, lambda: eng.encdec_tokens_full(mel, ids_stride=P))
    # rows of 32 ids cannot hold the result
    dev = DevBuf(mel)
    refused(UNSUPPORTED, lambda: eng.encdec_tokens_batch(mel))
    refused(UNSUPPORTED, lambda: eng.encdec_tokens_batch_dev(dev.data_ptr(), 3))
    refused(UNSUPPORTED, lambda: eng.transcribe_tokens_batch_dev(dev.data_ptr(), 3))
    refused(UNSUPPORTED, lambda: eng.encdec_debug_batch(mel, want_enc_out=False, want_logits=True))  # the logits tap
    refused(UNSUPPORTED, lambda: eng.encdec_debug_batch(mel, want_enc_out=True, want_logits=False))
    # the pipeline
    refused(UNSUPPORTED, lambda: eng.pipeline_submit_dev(dev.data_ptr(), 3))
    pcm_dev = DevBuf(np.zeros((1, eng.pcm_len), np.float32))
    refused(UNSUPPORTED, lambda: eng.pipeline_submit_pcm_dev(pcm_dev.data_ptr(), 1))
    pcm_dev.free()
    eng._submitted = []
    assert eng.get_option("in_flight") == 0
    dev.free()
    # beam search, bf16 storage, automatic language, forced ids
    eng.set_option("beam_size", 4)
    refused(UNSUPPORTED, lambda: eng.encdec_tokens_full(mel))
    eng.set_option("beam_size", 1)
    eng.set_option("bf16", 1)
    refused(UNSUPPORTED, lambda: eng.encdec_tokens_full(mel))
    eng.set_option("bf16", 0)
    eng.set_option("language", pkg.WT_LANGUAGE_AUTO)
    refused(UNSUPPORTED, lambda: eng.encdec_tokens_full(mel))
    refused(UNSUPPORTED, lambda: eng.transcribe(np.zeros(1600, np.float32)))
    eng.set_option("language", 2)
    forced = np.zeros((3, 32), np.int64)
    forced[:, :4] = fm.RICH_PROMPT
    L = pkg.lib()
    assert L.wt_dbg_set_forced_ids(eng.handle, forced.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 3) == 0
    refused(UNSUPPORTED, lambda: eng.encdec_tokens_full(mel))  # (refused() switches the tap off again)
    # everything restored: a full-length call works
    ids, n = eng.encdec_tokens_full(mel)
    assert ids.shape == (3, P + 1) and np.array_equal(ids[:, :4], np.tile(fm.RICH_PROMPT, (3, 1)))
    eng.close()


def test_monolith_engine_may_use_the_option(pkg, rich, rich_mel):
    eng = pkg.Engine(rich[0], rich[1], True, engine_type=pkg.EngineType.Monolith)
    eng.set_option("max_positions", 64)
    ids, n = eng.encdec_tokens_full(np.ascontiguousarray(rich_mel[:2]))
    assert ids.shape == (2, 65) and (n >= 5).all() and (n <= 65).all()
    assert ids[0, 0] == eng.vocab_info()["sot"]
    eng.close()


def test_tiny_end_to_end(pkg, orc, assets):
    """d = 384 and 6 heads end to end: synthetic tiny weights, 2 clips, P = 96, against the oracle under the margin rule."""
    prefix, vocab = assets("tiny")
    eng = pkg.Engine(prefix, vocab, True)
    assert eng.dims.n_text_ctx == 448
    eng.set_option("max_positions", 96)
    mel = fm.mels(2, eng.mel_shape, 5)
    ids, n = eng.encdec_tokens_full(mel)
    model = orc.Model(prefix + ".wtw")
    ref = fm.oracle_rows(model, mel, fm.RICH_PROMPT, 96, fm.EOT)
    model.close()
    # (on the oracle no step of these two clips has a margin below 7e-4: nothing may be set aside)
    aside = compare_with_margin_rule(rows_of(ids, n), ref, len(fm.RICH_PROMPT), max_aside=0)
    print("tiny clips set aside (clip, index):", aside, "smallest margins:", [float(m.min()) for _, m in ref])
    eng.set_option("max_positions", 0)
    ids31, n31 = eng.encdec_tokens_batch(mel)
    assert np.array_equal(ids[:, :31], ids31[:, :31])
    eng.close()
