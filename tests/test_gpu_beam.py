"""Beam search (option beam_size) on the GPU against the Python reference of tests/beam_ref.py
over the CPU oracle's logits.  Without the feature set_option("beam_size", K > 1) is WT_ERR_INVALID_ARG, so every test
here fails."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_model  # noqa: E402
import beam_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DELTA = 2e-4  # decision margin and score tolerance: 7x the largest measured sum error
# beam_model.write_eot_rich (eot_gain, gain, n_active): on micro about half of the clips finish before max length, most
# of them with EOTs from several slots; on tiny the same construction with fewer, longer active rows
MICRO_RICH = (3.3, 40.0, 64)
TINY_RICH = (3.0, 60.0, 32)
MICRO_PROMPT = [3, 5, 7, 11]  # the micro vocabulary (1024) has no multilingual special ids
UNSUPPORTED, INVALID = 4, 1


def mels(n, shape, seed=1234):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.5, size=(n,) + tuple(shape)).astype(np.float32)


def code_of(exc):
    return {"WT_ERR_UNSUPPORTED": UNSUPPORTED, "WT_ERR_INVALID_ARG": INVALID}.get(str(exc.value).split(":")[0])


@pytest.fixture(scope="module")
def eot_rich(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("beam") / "micro-eot-rich")
    eot_gain, gain, n_active = MICRO_RICH
    beam_model.write_eot_rich(prefix + ".wtw", p + ".wtw", eot_gain, gain, n_active)
    return p, vocab


@pytest.fixture(scope="module")
def tiny_rich(assets, tmp_path_factory):
    prefix, vocab = assets("tiny")
    p = str(tmp_path_factory.mktemp("beam") / "tiny-eot-rich")
    eot_gain, gain, n_active = TINY_RICH
    beam_model.write_eot_rich(prefix + ".wtw", p + ".wtw", eot_gain, gain, n_active)
    return p, vocab


def test_option_surface_and_scope_cuts(pkg, assets):
    from conftest import DevBuf
    import ctypes
    prefix, vocab = assets("micro")
    eng = pkg.Engine(prefix, vocab, True)
    eng.set_prompt(MICRO_PROMPT)
    assert eng.get_option("beam_size") == 1
    for k in range(1, 9):
        eng.set_option("beam_size", k)
        assert eng.get_option("beam_size") == k
    for bad in (0, 9):
        with pytest.raises(pkg.WtError) as e:
            eng.set_option("beam_size", bad)
        assert code_of(e) == INVALID
    mel = mels(2, eng.mel_shape)
    eng.set_option("beam_size", 1)
    eng.encdec_tokens_batch(mel)
    with pytest.raises(pkg.WtError):  # the last call was greedy
        eng.last_beam_scores()
    eng.set_option("beam_size", 4)
    ids, n = eng.encdec_tokens_batch(mel)
    sums, lens = eng.last_beam_scores()
    assert sums.shape == (2,) and list(lens) == [int(x) - len(MICRO_PROMPT) for x in n]

    def unsupported(fn):
        with pytest.raises(pkg.WtError) as e:
            fn()
        assert code_of(e) == UNSUPPORTED, str(e.value)

    dev = DevBuf(mel)
    unsupported(lambda: eng.pipeline_submit_dev(dev.data_ptr(), 2))
    eng._submitted = []
    unsupported(lambda: eng.encdec_debug_batch(mel, want_enc_out=False, want_logits=True))
    for key, on, off in (("bf16", 1, 0), ("cross_absorb", 0, 1), ("stop_at_eot", 0, 1)):
        eng.set_option(key, on)
        unsupported(lambda: eng.encdec_tokens_batch(mel))
        eng.set_option(key, off)
    L = pkg.lib()
    forced = np.zeros((2, 32), np.int64)
    forced[:, :4] = MICRO_PROMPT
    assert L.wt_dbg_set_forced_ids(eng.handle, forced.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 2) == 0
    unsupported(lambda: eng.encdec_tokens_batch(mel))
    assert L.wt_dbg_set_forced_ids(eng.handle, None, 0) == 0
    ids2, n2 = eng.encdec_tokens_batch(mel)  # everything restored: the same beam result again
    assert np.array_equal(ids, ids2) and np.array_equal(n, n2)
    dev.free()
    eng.close()


@pytest.mark.parametrize("batch", [8, 40])
def test_greedy_untouched(pkg, eot_rich, batch):
    prefix, vocab = eot_rich
    mel = mels(batch, (80, 200), seed=99)
    ref = pkg.Engine(prefix, vocab, True)  # never sees the option
    ids_ref, n_ref = ref.encdec_tokens_batch(mel)
    ref.close()
    eng = pkg.Engine(prefix, vocab, True)
    eng.set_option("beam_size", 1)
    ids, n = eng.encdec_tokens_batch(mel)
    assert np.array_equal(ids, ids_ref) and np.array_equal(n, n_ref)
    eng.set_option("beam_size", 4)
    eng.encdec_tokens_batch(mel)
    eng.set_option("beam_size", 1)
    ids, n = eng.encdec_tokens_batch(mel)
    assert np.array_equal(ids, ids_ref) and np.array_equal(n, n_ref)
    eng.close()


def check_parity(eng, model, mel, K, max_tokens, fns):
    """Runs the batch at K on the engine and the reference per clip; returns the reference results."""
    eng.set_option("beam_size", K)
    eng.set_option("max_tokens", max_tokens)
    ids, n = eng.encdec_tokens_batch(mel)
    sums, lens = eng.last_beam_scores()
    prompt = beam_model.PROMPT
    max_pos = min(max(max_tokens, len(prompt)), 31)
    refs, decisive = [], 0
    for b in range(mel.shape[0]):
        if b not in fns:
            fns[b] = beam_ref.oracle_logits_fn(model, model.encode(mel[b]), beam_model.EOT)
        r = beam_ref.beam_search(fns[b], prompt, K, max_pos, beam_model.EOT)
        refs.append(r)
        got = [int(x) for x in ids[b, : n[b]]]
        assert lens[b] == n[b] - len(prompt), (b, lens[b], n[b])
        # every clip: the reported sum is the sum of the engine's own ids under the oracle
        tf = beam_ref.teacher_forced_sum(fns[b], got, len(prompt))
        assert abs(sums[b] - tf) < DELTA, (K, max_tokens, b, sums[b], tf)
        if r["margin"] > DELTA:
            decisive += 1
            assert got == r["ids"], (K, max_tokens, b, got, r["ids"], r["margin"])
            assert abs(sums[b] - r["sum"]) < DELTA, (K, max_tokens, b, sums[b], r["sum"])
    assert decisive >= 0.9 * mel.shape[0], (K, max_tokens, decisive)
    return refs


def test_parity_eot_rich_micro(pkg, orc, eot_rich):
    prefix, vocab = eot_rich
    model = orc.Model(prefix + ".wtw")
    eng = pkg.Engine(prefix, vocab, True)
    assert eng.vocab_info()["eot"] == beam_model.EOT
    mel = mels(48, eng.mel_shape)
    fns = {}
    refs = check_parity(eng, model, mel, 4, 30, fns)  # 192 rows: two chains of 32 clips
    early = sum(r["done_early"] for r in refs)
    assert early >= 0.25 * len(refs) and len(refs) - early >= 0.25 * len(refs), early
    assert any(s != 0 for r in refs for s in r["eot_slots"])
    sub = mel[:16]
    sub_fns = {b: fns[b] for b in range(16)}
    for K in (2, 5, 8):
        for max_tokens in (30, 10):
            check_parity(eng, model, sub, K, max_tokens, sub_fns)
    eng.close()
    model.close()


def test_parity_fc2_ksplit_1(pkg, orc, eot_rich):
    """The chains share one decoder pass: beam search with fc2 unsplit (fc2_ksplit = 1, x handed from layer to layer and
    to the logits GEMM whole instead of as two halves), 8 clips at beam_size 2, held to the same reference."""
    prefix, vocab = eot_rich
    model = orc.Model(prefix + ".wtw")
    eng = pkg.Engine(prefix, vocab, True)
    eng.set_option("fc2_ksplit", 1)
    assert eng.get_option("fc2_ksplit") == 1
    check_parity(eng, model, mels(8, eng.mel_shape), 2, 30, {})
    eng.close()
    model.close()


def test_parity_tiny(pkg, orc, tiny_rich):
    prefix, vocab = tiny_rich
    model = orc.Model(prefix + ".wtw")
    eng = pkg.Engine(prefix, vocab, True)
    check_parity(eng, model, mels(3, eng.mel_shape, seed=5), 5, 30, {})
    eng.close()
    model.close()


def test_entry_points_agree(pkg, eot_rich):
    prefix, vocab = eot_rich
    eng = pkg.Engine(prefix, vocab, True)
    eng.set_option("beam_size", 5)
    rng = np.random.default_rng(42)
    pcm = (0.1 * rng.standard_normal((3, eng.pcm_len))).astype(np.float32)
    mel = eng.logmel_batch(pcm)
    ids, n = eng.encdec_tokens_batch(mel)
    texts = [eng.transcribe(pcm[b]) for b in range(3)]
    for b in range(3):
        assert texts[b] == eng.decode_text(ids[b, : n[b]])
    assert eng.transcribe_long(pcm.reshape(-1)) == "\n".join(texts)
    # graphs: the second call replays the captured chains; eager launches give the same ids and scores
    mel8 = mels(40, eng.mel_shape, seed=3)
    a = eng.encdec_tokens_batch(mel8)
    b = eng.encdec_tokens_batch(mel8)
    sa = eng.last_beam_scores()
    eng.set_option("use_graphs", 0)
    c = eng.encdec_tokens_batch(mel8)
    sc = eng.last_beam_scores()
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])
    assert np.array_equal(sa[0], sc[0]) and np.array_equal(sa[1], sc[1])
    eng.close()
