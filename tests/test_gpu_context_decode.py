"""A context in front of the prompt (wt_engine_set_context) on the GPU against the references of
tests/ts_ref.py, tests/scores_ref.py and tests/sample_ref.py over the CPU oracle, which decodes behind a prompt of any
length: the fed prompt is [prev] + the last n_text_ctx / 2 - 1 context ids + the engine's prompt.  Models of
tests/ts_model.py, tests/full_model.py and tests/scores_model.py.  Without the feature Engine.set_context does not exist
and every test here fails."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import full_model as fm  # noqa: E402
import sample_ref  # noqa: E402
import scores_model as sm  # noqa: E402
import scores_ref  # noqa: E402
import ts_model as tm  # noqa: E402
import ts_ref  # noqa: E402
from conftest import DevBuf  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = "WT_ERR_UNSUPPORTED", "WT_ERR_INVALID_ARG"
PREV = 50361                       # <|startofprev|> of the multilingual vocabulary
P_TS, KEEP_TS = tm.N_TEXT_CTX, tm.N_TEXT_CTX // 2 - 1      # 128 positions, 63 context ids kept
P_PLAIN, KEEP_PLAIN = fm.N_TEXT_CTX, fm.N_TEXT_CTX // 2 - 1  # 160, 79
CLIPS = 3                          # distinct clips; larger batches repeat them
LENGTHS = (1, 4, 27, KEEP_TS, 200)  # 27: the fed prompt ends at position 31 / 32; 200: truncated to the last 63
TOKEN_BOUND = 1.1e-4               # tests/test_gpu_scores.py: five times the largest measured |lp - reference lp|
MARGIN = tm.MARGIN


def status_of(exc):
    return str(exc.value).split(":")[0]


def context(n):
    """n ids: text ids, the special ids a transcript never holds left out, and a few timestamps as seeking feeds them."""
    rng = np.random.default_rng(100 + n)
    ids = rng.integers(0, tm.EOT, size=n)
    ids[rng.random(n) < 0.15] = tm.BEG + rng.integers(0, 100)
    return [int(i) for i in ids]


def fed(ctx, prompt, keep):
    return [PREV] + ctx[-keep:] + list(prompt)


@pytest.fixture(scope="module")
def models(assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    d = tmp_path_factory.mktemp("context")
    ts, plain = str(d / "micro-ctx-ts"), str(d / "micro-ctx-plain")
    sm.write_ts_model(prefix + ".wtw", ts + ".wtw")      # the timestamp model with a <|nospeech|> row that matters
    sm.write_plain_model(prefix + ".wtw", plain + ".wtw")
    return {"ts": (ts, vocab), "plain": (plain, vocab)}


@pytest.fixture(scope="module")
def mels():
    out = {"ts": np.ascontiguousarray(sm.ts_mels()[:CLIPS]), "plain": np.ascontiguousarray(sm.plain_mels()[:CLIPS])}
    for m in out.values():
        m.setflags(write=False)
    return out


class Reference:
    """Rows of the reference, each computed once on demand and never changed: scores_ref-style dicts with ids, lps, sum,
    n, avg, no_speech_prob (behind fed[: index(sot) + 1]) and first (the first indecisive step, or None)."""

    def __init__(self, orc, models, mels):
        self.models = {k: orc.Model(v[0] + ".wtw") for k, v in models.items()}
        self.mels, self.enc, self.rows = mels, {}, {}

    def close(self):
        for m in self.models.values():
            m.close()

    def row(self, mode, clip, n_ctx):
        key = (mode, clip, n_ctx)
        if key in self.rows:
            return self.rows[key]
        ts = mode == "ts"
        model, P = self.models[mode], P_TS if ts else P_PLAIN
        prompt = fed(context(n_ctx), sm.TS_PROMPT if ts else sm.PLAIN_PROMPT, KEEP_TS if ts else KEEP_PLAIN)
        if (mode, clip) not in self.enc:
            self.enc[(mode, clip)] = model.encode(self.mels[mode][clip])
        fn = tm.logits_fn(model, self.enc[(mode, clip)], P)
        n0, n_tail = len(prompt), len(sm.TS_PROMPT if ts else sm.PLAIN_PROMPT)
        nsp = scores_ref.no_speech_prob(fn(prompt[: n0 - n_tail + 1]), sm.NOSP)
        ids, lps, first = list(prompt), [], None
        while len(ids) <= P:
            z = np.asarray(fn(ids), np.float32)
            g = ids[n0:]
            if ts:
                tok, info = ts_ref.step(z, g, tm.EOT, tm.BEG)
                gap = min(info["gap_lm"], info["gap_top"])
            else:
                allowed = np.ones(z.size, bool)
                tok, gap = ts_ref._argmax_last(z, allowed), ts_ref._top_two_gap(z, allowed)
            if first is None and gap <= MARGIN:
                first = len(lps)
            lps.append(scores_ref.token_logprob(z, tok, g, tm.EOT, tm.BEG, 50, ts)[0])
            ids.append(tok)
            if tok == tm.EOT:
                break
        total = float(np.sum(np.asarray(lps, np.float64)))
        self.rows[key] = {"ids": ids, "n0": n0, "lps": lps, "sum": total, "n": len(lps), "avg": total / len(lps),
                          "no_speech_prob": nsp, "first": first}
        return self.rows[key]


@pytest.fixture(scope="module")
def ref(orc, models, mels):
    r = Reference(orc, models, mels)
    yield r
    r.close()


def new_engine(pkg, models, mode, **options):
    eng = pkg.Engine(models[mode][0], models[mode][1], True)
    eng.set_option("max_positions", P_TS if mode == "ts" else P_PLAIN)
    eng.set_option("timestamps", 1 if mode == "ts" else 0)
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


@pytest.fixture(scope="module")
def engs(pkg, models):
    e = {mode: new_engine(pkg, models, mode) for mode in ("ts", "plain")}
    info = e["ts"].vocab_info()
    assert (info["prev"], info["eot"], info["beg"]) == (PREV, tm.EOT, tm.BEG)
    assert e["ts"].dims.n_text_ctx == tm.N_TEXT_CTX and e["plain"].dims.n_text_ctx == fm.N_TEXT_CTX
    yield e
    for x in e.values():
        x.close()


def decode(eng, mel, pick):
    ids, n = eng.encdec_tokens_full(np.ascontiguousarray(mel[list(pick)]))
    return [[int(x) for x in ids[b, : n[b]]] for b in range(len(pick))]


def check(rows, ref, mode, pick, n_ctx):
    """Ids and counts equal the reference on every decisive clip; an indecisive clip up to its first indecisive step."""
    assert len(rows) == len(pick)
    for got, b in zip(rows, pick):
        r = ref.row(mode, b, n_ctx)
        assert got[: r["n0"]] == r["ids"][: r["n0"]], (b, "the fed prompt")
        if r["first"] is None:
            assert got == r["ids"], (mode, b, n_ctx)
        else:
            assert r["first"] >= 1 and got[: r["n0"] + r["first"]] == r["ids"][: r["n0"] + r["first"]], (mode, b, n_ctx)


@pytest.mark.parametrize("n_ctx", LENGTHS)
def test_ids_and_counts_equal_the_reference_behind_the_fed_prompt(engs, mels, ref, n_ctx):
    eng = engs["ts"]
    eng.set_context(context(n_ctx))
    assert eng.get_option("context_ids") == min(n_ctx, KEEP_TS)
    pick = [0, 1, 2, 0, 1]
    rows = decode(eng, mels["ts"], pick)
    check(rows, ref, "ts", pick, n_ctx)
    assert rows[0][0] == PREV and rows[0][1: 1 + min(n_ctx, KEEP_TS)] == context(n_ctx)[-KEEP_TS:]
    assert decode(eng, mels["ts"], pick) == rows          # again: the same ids
    assert decode(eng, mels["ts"], [1]) == [rows[1]]      # one clip: the cached cross-attention, 128 positions a pass
    eng.set_context([])
    assert eng.get_option("context_ids") == 0


def test_the_references_are_decisive(ref):
    """Most rows compared above are compared whole."""
    rows = [ref.row("ts", b, n) for n in LENGTHS for b in range(CLIPS)]
    whole = sum(1 for r in rows if r["first"] is None)
    print("rows compared whole:", whole, "of", len(rows), "lengths:", [len(r["ids"]) - r["n0"] for r in rows])
    assert whole * 4 >= len(rows) * 3
    assert max(len(r["ids"]) - r["n0"] for r in rows) > 8  # ... and they generate past the prompt


@pytest.mark.parametrize("n_ctx", [4, 200])
def test_without_timestamps(engs, mels, ref, n_ctx):
    eng = engs["plain"]
    eng.set_context(context(n_ctx))
    assert eng.get_option("context_ids") == min(n_ctx, KEEP_PLAIN)
    check(decode(eng, mels["plain"], [0, 1, 2]), ref, "plain", [0, 1, 2], n_ctx)
    eng.set_context([])


@pytest.mark.parametrize("n_ctx", [27, KEEP_TS])
def test_batches_cross_attention_forms_eager_and_prompt_group(pkg, models, mels, ref, n_ctx):
    """1, 5, 32 and 40 clips; 32 and more take the absorbed cross-attention (the cached one with cross_absorb = 0:
    four positions a pass, one launch); use_graphs 0 and 1; prompt_group 0 and 1."""
    e = new_engine(pkg, models, "ts")
    assert e.get_option("cross_absorb_active") == 1
    e.set_context(context(n_ctx))
    mel = mels["ts"]
    p32, p40 = [b % CLIPS for b in range(32)], [b % CLIPS for b in range(40)]
    r32 = decode(e, mel, p32)
    check(r32, ref, "ts", p32, n_ctx)
    check(decode(e, mel, p40), ref, "ts", p40, n_ctx)
    e.set_option("prompt_group", 1)
    assert e.get_option("prompt_group") == 1
    assert decode(e, mel, p32) == r32
    check(decode(e, mel, [2]), ref, "ts", [2], n_ctx)
    check(decode(e, mel, [0, 1, 2, 0, 1]), ref, "ts", [0, 1, 2, 0, 1], n_ctx)
    e.set_option("prompt_group", 0)
    e.set_option("cross_absorb", 0)
    check(decode(e, mel, p32), ref, "ts", p32, n_ctx)
    e.set_option("use_graphs", 0)
    check(decode(e, mel, p32), ref, "ts", p32, n_ctx)
    check(decode(e, mel, [2]), ref, "ts", [2], n_ctx)
    e.set_option("cross_absorb", 1)
    assert decode(e, mel, p32) == r32
    for bad in (-1, 2):
        with pytest.raises(pkg.WtError) as err:
            e.set_option("prompt_group", bad)
        assert status_of(err) == INVALID
    e.close()


def test_graphs_cached_does_not_grow_with_the_context_lengths_seen(pkg, models, mels):
    e = new_engine(pkg, models, "ts")
    one = np.ascontiguousarray(mels["ts"][:1])
    plain_ids = e.encdec_tokens_full(one)   # no context: the segment graphs of this call are captured
    held = e.get_option("graphs_cached")
    assert held >= 1
    for n_ctx in (1, 2, 3, 5, 8, 13, 21, 34, 55, 60, 61, 62):
        e.set_context(context(n_ctx))
        e.encdec_tokens_full(one)
        assert e.get_option("graphs_cached") == held, n_ctx
    e.set_context([])
    again = e.encdec_tokens_full(one)       # ... and they are still the ones replayed
    assert e.get_option("graphs_cached") == held
    assert np.array_equal(again[0], plain_ids[0]) and np.array_equal(again[1], plain_ids[1])
    e.close()


def test_clearing_the_context_restores_the_engine_bit_for_bit(pkg, models, mels):
    three = mels["ts"]
    fresh = new_engine(pkg, models, "ts", scores=1)  # never had a context
    want = (*fresh.encdec_tokens_full(three), fresh.last_scores(), fresh.last_token_logprobs(P_TS + 1))
    fresh.close()
    e = new_engine(pkg, models, "ts", scores=1)
    e.set_context(context(27))
    e.encdec_tokens_full(three)
    e.set_context([])
    got = (*e.encdec_tokens_full(three), e.last_scores(), e.last_token_logprobs(P_TS + 1))
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    e.set_option("prompt_group", 1)  # changes nothing without a context
    got = (*e.encdec_tokens_full(three), e.last_scores(), e.last_token_logprobs(P_TS + 1))
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    e.close()


@pytest.mark.parametrize("mode,n_ctx", [("ts", 4), ("ts", 27), ("ts", 200), ("plain", 4)])
def test_scores_behind_a_context(pkg, models, mels, ref, mode, n_ctx):
    """The bars of tests/test_gpu_scores.py; the no-speech probability is read at sot's position in the fed prompt."""
    e = new_engine(pkg, models, mode, scores=1)
    e.set_context(context(n_ctx))
    for pick in ([0, 1, 2, 0, 1], [1], [b % CLIPS for b in range(32)]):
        ids, n = e.encdec_tokens_full(np.ascontiguousarray(mels[mode][pick]))
        sc, lp = e.last_scores(), e.last_token_logprobs(ids.shape[1])
        for row, b in enumerate(pick):
            r = ref.row(mode, b, n_ctx)
            n0, k = r["n0"], r["n"] if r["first"] is None else r["first"]
            assert [int(x) for x in ids[row, : n0 + k]] == r["ids"][: n0 + k], (b, row)
            rel = abs(sc["no_speech_prob"][row] - r["no_speech_prob"]) / r["no_speech_prob"]
            print(f"{mode} ctx {n_ctx} clip {b}: no_speech_prob {sc['no_speech_prob'][row]:.6g} (reference {r['no_speech_prob']:.6g})")
            assert rel <= TOKEN_BOUND + 2.0 ** -23, (b, rel)
            assert not lp[row, :n0].any()   # 0 for the whole fed prompt
            err = float(np.abs(lp[row, n0: n0 + k].astype(np.float64) - np.asarray(r["lps"][:k], np.float64)).max())
            assert err <= TOKEN_BOUND, (b, err)
            if k < r["n"]:
                continue
            assert n[row] == len(r["ids"]) and sc["n_generated"][row] == r["n"] and not lp[row, n[row]:].any()
            assert abs(sc["sum_logprob"][row] - r["sum"]) <= TOKEN_BOUND * r["n"] + abs(r["sum"]) * 2.0 ** -23
            assert abs(sc["avg_logprob"][row] - r["avg"]) <= TOKEN_BOUND + abs(r["avg"]) * 2.0 ** -23
    e.close()


def test_the_no_speech_row_moves_with_the_context(ref):
    """The reference's no-speech probability behind [prev] + context + [sot] is not the one behind [sot] alone, so an
    engine that read position 0 would miss it."""
    with_ctx = [ref.row("ts", b, 27)["no_speech_prob"] for b in range(CLIPS)]
    model = ref.models["ts"]
    alone = [scores_ref.no_speech_prob(tm.logits_fn(model, ref.enc[("ts", b)], P_TS)(sm.TS_PROMPT[:1]), sm.NOSP) for b in range(CLIPS)]
    print(with_ctx, alone)
    assert any(abs(a - b) > 100 * TOKEN_BOUND * b for a, b in zip(with_ctx, alone))


def test_sampling_behind_a_context(pkg, orc, models, mels, ref):
    """One temperature: sample_ref.decode is driven with the longer prompt as it stands (its position word is the id's
    position in the fed row)."""
    milli, seed, n_ctx = 200, 1, 27
    e = new_engine(pkg, models, "ts", scores=1, temperature=milli, seed=seed)
    e.set_context(context(n_ctx))
    pick = [0, 1, 2]
    ids, n = e.encdec_tokens_full(np.ascontiguousarray(mels["ts"][pick]))
    info = e.last_decode_info()
    model = ref.models["ts"]
    prompt = fed(context(n_ctx), sm.TS_PROMPT, KEEP_TS)
    n0 = len(prompt)
    for row, b in enumerate(pick):
        fn = tm.logits_fn(model, ref.enc[("ts", b)] if ("ts", b) in ref.enc else model.encode(mels["ts"][b]), P_TS)
        r = sample_ref.decode(fn, prompt, P_TS, tm.EOT, sm.NOSP, sample_ref.temperature_of_milli(milli), seed, clip=row, beg=tm.BEG,
                              timestamps=True)
        s = sample_ref.first_indecisive(r["infos"], 2 * 1e-4 / (milli / 1000.0))  # the key bar plus twice the logits bar over T
        k = r["n"] if s is None else s
        assert k >= 1 and [int(x) for x in ids[row, : n0 + k]] == r["ids"][: n0 + k], b
        assert info["temperature_milli"][row] == milli
        if s is None:
            assert n[row] == len(r["ids"])
    e.close()


def test_refusals_leave_the_engine_usable(pkg, models, mels, assets):
    e = new_engine(pkg, models, "ts")
    one = np.ascontiguousarray(mels["ts"][:1])
    want = e.encdec_tokens_full(one)

    def refused(fn, status=UNSUPPORTED, word="context"):
        with pytest.raises(pkg.WtError) as err:
            fn()
        assert status_of(err) == status, str(err.value)
        if word:
            assert word in str(err.value)

    # what set_context itself refuses
    refused(lambda: e.set_context([1, 2, tm.N_VOCAB]), INVALID)
    refused(lambda: e.set_context([-1]), INVALID)
    refused(lambda: e.set_context(np.zeros(4097, np.int64)), INVALID)
    assert e.get_option("context_ids") == 0
    e.set_context(np.arange(4096))  # the most it takes: the last 63 are kept
    assert e.get_option("context_ids") == KEEP_TS
    e.set_context(context(4))
    pcm = np.zeros(e.pcm_len, np.float32)
    # a [B][32] call, a pipelined call (both refused with max_positions set, as ever), then calls without max_positions
    refused(lambda: e.encdec_tokens_batch(one), word=None)
    d_mel = DevBuf(one)
    try:
        refused(lambda: e.pipeline_submit_dev(d_mel.data_ptr(), 1), word=None)
        e.set_option("timestamps", 0)
        e.set_option("max_positions", 0)
        refused(lambda: e.encdec_tokens_batch(one))
        refused(lambda: e.transcribe(pcm))
        refused(lambda: e.transcribe_long(pcm))
        refused(lambda: e.pipeline_submit_dev(d_mel.data_ptr(), 1))
        refused(lambda: e.encdec_debug_batch(one))
    finally:
        d_mel.free()
    e.set_option("max_positions", P_TS)
    e.set_option("timestamps", 1)
    # beam search, the bf16 storage mode, automatic language, forced ids: refused by full-length decoding with its own text
    e.set_option("beam_size", 2)
    refused(lambda: e.encdec_tokens_full(one), word=None)
    e.set_option("beam_size", 1)
    e.set_option("bf16", 1)
    refused(lambda: e.encdec_tokens_full(one), word=None)
    e.set_option("bf16", 0)
    language = e.get_option("language")
    e.set_option("language", -1)
    refused(lambda: e.encdec_tokens_full(one), word=None)
    e.set_option("language", language)
    e.set_forced_ids(np.zeros((1, 32), np.int64))
    refused(lambda: e.encdec_tokens_full(one), word=None)
    e.set_forced_ids(None)
    # a prompt that leaves no position to generate
    e.set_context(context(KEEP_TS))
    e.set_option("max_positions", 1 + KEEP_TS + len(tm.PROMPT))
    refused(lambda: e.encdec_tokens_full(one), INVALID)
    e.set_option("max_positions", 2 + KEEP_TS + len(tm.PROMPT))
    ids, n = e.encdec_tokens_full(one)   # one prompt-free position left: max_positions + 1 ids, or one fewer behind an EOT
    full = 2 + KEEP_TS + len(tm.PROMPT) + 1
    assert n[0] == (full - 1 if ids[0, full - 2] == tm.EOT else full)
    assert [int(v) for v in ids[0, : full - 2]] == fed(context(KEEP_TS), tm.PROMPT, KEEP_TS)
    e.set_option("max_positions", P_TS)
    e.set_context([])
    got = e.encdec_tokens_full(one)      # ... and the engine is as it was
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    e.close()
    # a vocabulary without <|startofprev|>, a Monolith engine
    prefix, vocab = assets("micro")
    m = pkg.Engine(prefix, vocab, True)
    refused(lambda: m.set_context([1, 2, 3]))
    m.set_context([])  # clearing is always allowed
    m.close()
    mono = pkg.Engine(models["ts"][0], models["ts"][1], True, pkg.EngineType.Monolith)
    refused(lambda: mono.set_context([1, 2, 3]))
    mono.close()
