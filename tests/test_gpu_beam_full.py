"""Full-length beam search (options full_beam + beam_size + max_positions) on the GPU against
tests/beam_full_ref.py over the CPU oracle, on the models of tests/ts_model.py (timestamps) and tests/full_model.py (the
EOT-rich one, no timestamps); tests/test_beam_full_reference.py pins what the reference gives on them.  The reference of
a (model, K, P, max_initial_timestamp) is computed once per module.  Without the feature set_option("full_beam", 1) fails
and so does every test here."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_full_ref as bfr  # noqa: E402
import full_model as fm  # noqa: E402
import ts_model as tm  # noqa: E402
import ts_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DELTA = 2e-4  # decision margin and score tolerance
UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
N0 = len(tm.PROMPT)
P_RICH = 160


def status_of(exc):
    return str(exc.value).split(":")[0]


@pytest.fixture(scope="module")
def ts_files(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("beamfull") / "micro-ts")
    tm.write_model(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def rich_files(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("beamfull") / "micro-rich")
    fm.write_eot_rich(prefix + ".wtw", p + ".wtw")
    return p, vocab


@pytest.fixture(scope="module")
def ts_mel():
    m = tm.mels()
    m.setflags(write=False)
    return m


@pytest.fixture(scope="module")
def rich_mel():
    m = fm.mels(fm.RICH_CLIPS, (80, 200), fm.RICH_SEED)
    m.setflags(write=False)
    return m


class Reference:
    """beam_full_ref over the oracle: per (K, P, max_initial) the clips' results, computed once."""

    def __init__(self, orc, wtw, mel, prompt, timestamps):
        self.orc, self.wtw, self.mel, self.prompt, self.timestamps = orc, wtw, mel, prompt, timestamps
        self.rows = {}

    def fn(self, model, b):
        return bfr.level_logits_fn(model, model.encode(self.mel[b]), tm.EOT)

    def get(self, K, P, mit=50):
        key = (K, P, mit)
        if key not in self.rows:
            model = self.orc.Model(self.wtw)
            self.rows[key] = [bfr.beam_search(self.fn(model, b), self.prompt, K, P, tm.EOT, tm.BEG, self.timestamps, mit)
                              for b in range(self.mel.shape[0])]
            model.close()
        return self.rows[key]

    def teacher_forced(self, b, ids, mit=50):
        model = self.orc.Model(self.wtw)
        out = bfr.teacher_forced(self.fn(model, b), ids, len(self.prompt), tm.EOT, tm.BEG, self.timestamps, mit)
        model.close()
        return out


@pytest.fixture(scope="module")
def ts_reference(orc, ts_files, ts_mel):
    return Reference(orc, ts_files[0] + ".wtw", ts_mel, tm.PROMPT, True)


@pytest.fixture(scope="module")
def rich_reference(orc, rich_files, rich_mel):
    return Reference(orc, rich_files[0] + ".wtw", rich_mel, fm.RICH_PROMPT, False)


def new_engine(pkg, files, K, P, timestamps, **options):
    eng = pkg.Engine(files[0], files[1], True)
    eng.set_option("max_positions", P)
    eng.set_option("timestamps", int(timestamps))
    eng.set_option("beam_size", K)
    eng.set_option("full_beam", 1)
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


def check_parity(eng, reference, mel, K, P, mit=50, pick=None):
    """test_gpu_beam.py's pattern: every clip's reported sum is within DELTA of the oracle's teacher-forced float64 sum of
    the engine's own ids under A; decisive clips have the reference's ids, counts and sums; at least three quarters of the
    clips are decisive.  Returns (ids, n, the largest sum error seen)."""
    pick = list(range(mel.shape[0])) if pick is None else pick
    refs = reference.get(K, P, mit)
    n0 = len(reference.prompt)
    ids, n = eng.encdec_tokens_full(np.ascontiguousarray(mel[pick]))
    sums, lens = eng.last_beam_scores()
    assert ids.shape == (len(pick), P + 1)
    decisive, worst, seen = 0, 0.0, {}
    for i, b in enumerate(pick):
        r = refs[b]
        got = [int(x) for x in ids[i, : n[i]]]
        assert not ids[i, n[i]:].any() and got[:n0] == list(reference.prompt)
        assert lens[i] == n[i] - n0, (b, lens[i], n[i])
        if (b, tuple(got)) not in seen:  # (a clip repeated in the batch is teacher-forced once)
            seen[(b, tuple(got))] = math.fsum(r["lps"]) if got == r["ids"] else reference.teacher_forced(b, got, mit)[1]
        tf = seen[(b, tuple(got))]
        worst = max(worst, abs(float(sums[i]) - tf))
        print(f"K {K} P {P} mit {mit} clip {b}: n {n[i]} sum {sums[i]:.6f} teacher-forced {tf:.6f} margin {r['margin']:.2e}")
        assert abs(sums[i] - tf) < DELTA, (K, P, b, sums[i], tf)
        if r["margin"] > DELTA:
            decisive += 1
            assert got == r["ids"], (K, P, b, got, r["ids"], r["margin"])
            assert abs(sums[i] - r["sum"]) < DELTA, (K, P, b, sums[i], r["sum"])
    assert decisive * 4 >= 3 * len(pick), (K, P, decisive)
    print(f"K {K} P {P} mit {mit}: largest |sum - teacher-forced sum| {worst:.2e}")
    return ids, n, worst


@pytest.mark.parametrize("K,P", [(2, tm.P_LONG), (4, tm.P_LONG), (5, tm.P_SHORT)])
def test_parity_with_timestamps(pkg, ts_files, ts_mel, ts_reference, K, P):
    eng = new_engine(pkg, ts_files, K, P, True)
    info = eng.vocab_info()
    assert (info["eot"], info["beg"]) == (tm.EOT, tm.BEG)
    ids, n, _ = check_parity(eng, ts_reference, ts_mel, K, P)
    again = eng.encdec_tokens_full(ts_mel)  # the segment graphs replayed
    assert np.array_equal(again[0], ids) and np.array_equal(again[1], n)
    # the result differs from greedy decoding under the same rules
    eng.set_option("beam_size", 1)
    g_ids, g_n = eng.encdec_tokens_full(ts_mel)
    assert any(list(g_ids[b, : g_n[b]]) != list(ids[b, : n[b]]) for b in range(tm.CLIPS))
    eng.close()


def test_parity_without_timestamps(pkg, rich_files, rich_mel, rich_reference):
    eng = new_engine(pkg, rich_files, 4, P_RICH, False)
    check_parity(eng, rich_reference, rich_mel, 4, P_RICH)
    eng.close()


@pytest.mark.parametrize("mit,live", [(0, 1), (2, 3)])
def test_max_initial_timestamp_leaves_fewer_live_hypotheses(pkg, ts_files, ts_mel, ts_reference, mit, live):
    refs = ts_reference.get(4, tm.P_SHORT, mit)
    assert all(r["n_live"][:2] == [1, live] for r in refs)
    eng = new_engine(pkg, ts_files, 4, tm.P_SHORT, True, max_initial_timestamp=mit)
    ids, _, _ = check_parity(eng, ts_reference, ts_mel, 4, tm.P_SHORT, mit)
    assert ((ids[:, N0] >= tm.BEG) & (ids[:, N0] <= tm.BEG + mit)).all()
    eng.close()


def test_batch_sizes_graphs_and_replay(pkg, ts_files, ts_mel, ts_reference):
    """1, 5 and 64 clips (at K = 4, 64 clips are two chains of 32); with and without hipGraphs; replay."""
    K, P = 4, tm.P_LONG
    eng = new_engine(pkg, ts_files, K, P, True)
    pick64 = [b % tm.CLIPS for b in range(64)]
    a = check_parity(eng, ts_reference, ts_mel, K, P, pick=pick64)
    check_parity(eng, ts_reference, ts_mel, K, P, pick=[3])
    check_parity(eng, ts_reference, ts_mel, K, P, pick=list(range(5)))
    mel64 = np.ascontiguousarray(ts_mel[pick64])
    b = eng.encdec_tokens_full(mel64)  # replay
    sb = eng.last_beam_scores()
    eng.set_option("use_graphs", 0)
    c = eng.encdec_tokens_full(mel64)
    sc = eng.last_beam_scores()
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])
    assert np.array_equal(sb[0], sc[0]) and np.array_equal(sb[1], sc[1])
    check_parity(eng, ts_reference, ts_mel, K, P, pick=list(range(5)))  # eager
    eng.close()


def test_segments_scores_and_token_logprobs(pkg, ts_files, ts_mel, ts_reference):
    K, P = 4, tm.P_LONG
    refs = ts_reference.get(K, P)
    eng = new_engine(pkg, ts_files, K, P, True, scores=1)
    ids, n = eng.encdec_tokens_full(ts_mel)
    want = []
    for b in range(tm.CLIPS):
        want += ts_ref.segments(ids[b, : n[b]], N0, tm.EOT, tm.BEG, clip=b)
    segs = eng.last_segments()
    assert [tuple(int(x) for x in s) for s in segs] == want and len(want) >= tm.CLIPS
    scores = eng.last_scores()
    lps = eng.last_token_logprobs(P + 1)
    sums, lens = eng.last_beam_scores()
    greedy = pkg.Engine(ts_files[0], ts_files[1], True)  # the no-speech probability comes from the prompt pass: greedy's
    greedy.set_option("max_positions", P)
    greedy.set_option("timestamps", 1)
    greedy.set_option("scores", 1)
    greedy.encdec_tokens_full(ts_mel)
    g_scores = greedy.last_scores()
    greedy.close()
    decisive = 0
    for b, r in enumerate(refs):
        assert scores["n_generated"][b] == n[b] - N0 == lens[b]
        assert scores["sum_logprob"][b] == sums[b]
        assert abs(scores["avg_logprob"][b] - scores["sum_logprob"][b] / scores["n_generated"][b]) < 1e-6
        assert abs(scores["no_speech_prob"][b] - g_scores["no_speech_prob"][b]) < 1e-6
        assert not lps[b, :N0].any() and not lps[b, n[b]:].any()
        assert abs(float(lps[b, N0: n[b]].astype(np.float64).sum()) - scores["sum_logprob"][b]) < DELTA
        if r["margin"] > DELTA:
            decisive += 1
            assert [int(x) for x in ids[b, : n[b]]] == r["ids"]
            assert abs(scores["sum_logprob"][b] - r["sum"]) < DELTA
            assert np.abs(lps[b, N0: n[b]] - np.asarray(r["lps"])).max() < DELTA
    assert decisive * 4 >= 3 * tm.CLIPS
    # skip_silence follows on the host: with a threshold every clip exceeds, an unconfident clip is skipped
    eng.set_option("skip_silence", 1)
    eng.set_option("no_speech_threshold", 0)
    eng.set_option("logprob_threshold", 0)
    eng.encdec_tokens_full(ts_mel)
    assert eng.last_scores()["skipped"].all() and eng.last_segments().size == 0
    eng.close()


def test_text_entry_points_agree_with_the_ids(pkg, ts_files):
    eng = new_engine(pkg, ts_files, 4, tm.P_SHORT, True)
    rng = np.random.default_rng(42)
    pcm = (0.1 * rng.standard_normal((3, eng.pcm_len))).astype(np.float32)
    mel = eng.logmel_batch(pcm)
    ids, n = eng.encdec_tokens_full(mel)
    texts = [eng.transcribe(pcm[b]) for b in range(3)]
    for b in range(3):
        assert texts[b] == eng.decode_text(ids[b, : n[b]])
    assert eng.transcribe_long(pcm.reshape(-1)) == "\n".join(texts)
    eng.close()


def test_the_switch_and_the_old_paths(pkg, ts_files, ts_mel):
    """full_beam = 0 refuses as before; a 31-position beam call and a greedy full-length call give their old ids bit for
    bit after a full-beam call."""
    mel = np.ascontiguousarray(ts_mel[:4])
    old = pkg.Engine(ts_files[0], ts_files[1], True)  # never sees the option
    old.set_option("beam_size", 4)
    beam31 = old.encdec_tokens_batch(mel)
    beam31_scores = old.last_beam_scores()
    old.set_option("beam_size", 1)
    old.set_option("max_positions", tm.P_LONG)
    old.set_option("timestamps", 1)
    greedy = old.encdec_tokens_full(mel)
    old.set_option("beam_size", 4)
    with pytest.raises(pkg.WtError) as e:
        old.encdec_tokens_full(mel)
    assert status_of(e) == UNSUPPORTED and "full_beam" in str(e.value)
    old.close()

    eng = pkg.Engine(ts_files[0], ts_files[1], True)
    assert eng.get_option("full_beam") == 0
    for bad in (-1, 2):
        with pytest.raises(pkg.WtError) as e:
            eng.set_option("full_beam", bad)
        assert status_of(e) == INVALID
    eng.set_option("full_beam", 1)
    assert eng.get_option("full_beam") == 1
    eng.set_option("beam_size", 4)
    eng.set_option("max_positions", tm.P_LONG)
    eng.set_option("timestamps", 1)
    full = eng.encdec_tokens_full(mel)
    assert any(list(full[0][b]) != list(greedy[0][b]) for b in range(4))
    eng.set_option("beam_size", 1)
    got = eng.encdec_tokens_full(mel)
    assert np.array_equal(got[0], greedy[0]) and np.array_equal(got[1], greedy[1])
    eng.set_option("timestamps", 0)
    eng.set_option("max_positions", 0)
    eng.set_option("beam_size", 4)
    got = eng.encdec_tokens_batch(mel)
    assert np.array_equal(got[0], beam31[0]) and np.array_equal(got[1], beam31[1])
    got_scores = eng.last_beam_scores()
    assert np.array_equal(got_scores[0], beam31_scores[0]) and np.array_equal(got_scores[1], beam31_scores[1])
    eng.close()


def test_refusals_return_a_status_with_a_text(pkg, ts_files, ts_mel):
    from conftest import DevBuf
    mel = np.ascontiguousarray(ts_mel[:2])
    eng = new_engine(pkg, ts_files, 4, tm.P_SHORT, True)
    want = eng.encdec_tokens_full(mel)

    def unsupported(fn):
        with pytest.raises(pkg.WtError) as e:
            fn()
        assert status_of(e) == UNSUPPORTED and len(str(e.value)) > len(UNSUPPORTED) + 2, str(e.value)

    run = lambda: eng.encdec_tokens_full(mel)
    for key, on in (("temperature", 500), ("seek", 1), ("word_timestamps", 1), ("language", -1), ("bf16", 1),
                    ("stop_at_eot", 0), ("cross_absorb", 0)):
        off = eng.get_option(key)
        eng.set_option(key, on)
        unsupported(run)
        eng.set_option(key, off)
    eng.set_option("scores", 1)
    eng.set_option("temperature_fallback", 1)
    unsupported(run)
    eng.set_option("temperature_fallback", 0)
    eng.set_option("scores", 0)
    eng.set_context([5, 6, 7])
    unsupported(run)
    eng.set_context([])
    eng.set_contexts([[5, 6], [7]])
    unsupported(run)
    eng.set_contexts([])
    rng = np.random.default_rng(1)
    pcm = (0.1 * rng.standard_normal(eng.pcm_len)).astype(np.float32)
    unsupported(lambda: eng.transcribe_long_batch([pcm, pcm]))
    dev = DevBuf(mel)
    unsupported(lambda: eng.pipeline_submit_dev(dev.data_ptr(), 2))
    eng._submitted = []
    forced = np.zeros((2, 32), np.int64)
    forced[:, :N0] = tm.PROMPT
    L = pkg.lib()
    assert L.wt_dbg_set_forced_ids(eng.handle, forced.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 2) == 0
    unsupported(run)
    assert L.wt_dbg_set_forced_ids(eng.handle, None, 0) == 0
    got = run()  # the engine stays usable: the same result again
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    dev.free()
    eng.close()


def test_the_cli_sets_the_option_itself(pkg, ts_files, tmp_path):
    import struct
    import subprocess
    eng = new_engine(pkg, ts_files, 4, tm.P_SHORT, False)
    rng = np.random.default_rng(7)
    pcm16 = np.clip(np.round(0.1 * rng.standard_normal(eng.pcm_len) * 32767), -32768, 32767).astype("<i2")
    wav = tmp_path / "noise.wav"
    wav.write_bytes(b"RIFF" + struct.pack("<I", 36 + pcm16.nbytes) + b"WAVEfmt " +
                    struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" + struct.pack("<I", pcm16.nbytes) +
                    pcm16.tobytes())
    want = eng.transcribe(str(wav))
    eng.set_option("timestamps", 1)
    eng.transcribe(str(wav))
    segs, texts = eng.last_segments(with_text=True)
    eng.close()
    exe = os.path.join(ROOT, "whisper.tflite_amd", "bin", "encdec")
    base = [exe, "--model-prefix", ts_files[0], "--vocab", ts_files[1], "--input", str(wav), "--beam", "4",
            "--max-positions", str(tm.P_SHORT)]
    r = subprocess.run(base, capture_output=True, text=True, errors="replace", timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want + "\n"
    r = subprocess.run(base + ["--timestamps"], capture_output=True, text=True, errors="replace", timeout=120)
    assert r.returncode == 0, r.stderr
    stamp = lambda ms: "%02d:%02d.%03d" % (ms // 60000, ms // 1000 % 60, ms % 1000)
    assert len(texts) >= 1
    assert r.stdout == "".join("[%s --> %s] %s\n" % (stamp(int(s[1])), stamp(int(s[2])), t.decode("utf-8", errors="replace"))
                               for s, t in zip(segs, texts))
