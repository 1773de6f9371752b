"""Per-clip contexts (wt_engine_set_contexts) on the GPU: one ragged decoder chain over clips whose
fed prompts differ in length, against the references of tests/ts_ref.py, tests/scores_ref.py and tests/sample_ref.py over
the CPU oracle driven with each clip's OWN fed prompt.  Models, mels, contexts and bars are those of
tests/test_gpu_context_decode.py.  Without the feature Engine.set_contexts does not exist and every test here fails."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sample_ref  # noqa: E402
import scores_model as sm  # noqa: E402
import scores_ref  # noqa: E402
import test_gpu_context_decode as cd  # noqa: E402  (helpers and constants only)
import ts_model as tm  # noqa: E402
import ts_ref  # noqa: E402
from conftest import DevBuf  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = cd.UNSUPPORTED, cd.INVALID
PREV, CLIPS, TOKEN_BOUND, MARGIN = cd.PREV, cd.CLIPS, cd.TOKEN_BOUND, cd.MARGIN
P = {"ts": cd.P_TS, "plain": cd.P_PLAIN}
KEEP = {"ts": cd.KEEP_TS, "plain": cd.KEEP_PLAIN}
PROMPT = {"ts": sm.TS_PROMPT, "plain": sm.PLAIN_PROMPT}
LENGTHS = (0, 1, 27, 63, 200)  # per clip of one call; 200 is cut to the last n_text_ctx / 2 - 1


def status_of(exc):
    return str(exc.value).split(":")[0]


def context(n):
    return cd.context(n) if n else []


def fed(mode, n_ctx):
    ctx = context(n_ctx)
    return ([PREV] + ctx[-KEEP[mode]:] if ctx else []) + list(PROMPT[mode])


def layout(batch):
    """(clip, context length) of every row of a call: the lengths cycled, and the clips shifted against them."""
    return [((b + b // len(LENGTHS)) % CLIPS, LENGTHS[b % len(LENGTHS)]) for b in range(batch)]


models = cd.models
mels = cd.mels


class Reference:
    """cd.Reference's rows behind fed(mode, n_ctx), an empty context included; each computed once and never changed."""

    def __init__(self, orc, models, mels):
        self.models = {k: orc.Model(v[0] + ".wtw") for k, v in models.items()}
        self.mels, self.enc, self.rows = mels, {}, {}

    def close(self):
        for m in self.models.values():
            m.close()

    def logits_fn(self, mode, clip):
        if (mode, clip) not in self.enc:
            self.enc[(mode, clip)] = self.models[mode].encode(self.mels[mode][clip])
        return tm.logits_fn(self.models[mode], self.enc[(mode, clip)], P[mode])

    def row(self, mode, clip, n_ctx):
        key = (mode, clip, n_ctx)
        if key in self.rows:
            return self.rows[key]
        ts = mode == "ts"
        prompt = fed(mode, n_ctx)
        fn = self.logits_fn(mode, clip)
        n0, n_tail = len(prompt), len(PROMPT[mode])
        nsp = scores_ref.no_speech_prob(fn(prompt[: n0 - n_tail + 1]), sm.NOSP)
        ids, lps, first = list(prompt), [], None
        while len(ids) <= P[mode]:
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


@pytest.fixture(scope="module")
def engs(pkg, models):
    e = {mode: cd.new_engine(pkg, models, mode, scores=1) for mode in ("ts", "plain")}
    yield e
    for x in e.values():
        x.close()


def decode(eng, mel, rows):
    """One call over rows = [(clip, context length)]: per-clip contexts, then the id rows up to their counts."""
    eng.set_contexts([context(n) for _, n in rows])
    assert eng.get_option("context_clips") == len(rows) and eng.get_option("context_ids") == 0
    ids, n = eng.encdec_tokens_full(np.ascontiguousarray(mel[[c for c, _ in rows]]))
    return ids, n, [[int(x) for x in ids[b, : n[b]]] for b in range(len(rows))]


def check_scores(eng, ref, mode, rows, ids, n):
    """Section 15's bars, as tests/test_gpu_context_decode.py applies them, on every clip of the call."""
    sc, lp = eng.last_scores(), eng.last_token_logprobs(ids.shape[1])
    assert sc.size == len(rows)
    for row, (b, n_ctx) in enumerate(rows):
        r = ref.row(mode, b, n_ctx)
        n0, k = r["n0"], r["n"] if r["first"] is None else r["first"]
        rel = abs(sc["no_speech_prob"][row] - r["no_speech_prob"]) / r["no_speech_prob"]
        assert rel <= TOKEN_BOUND + 2.0 ** -23, (row, rel)
        assert not lp[row, :n0].any()   # 0 for the whole fed prompt
        err = float(np.abs(lp[row, n0: n0 + k].astype(np.float64) - np.asarray(r["lps"][:k], np.float64)).max())
        assert err <= TOKEN_BOUND, (row, err)
        if k < r["n"]:
            continue
        assert n[row] == len(r["ids"]) and sc["n_generated"][row] == r["n"] and not lp[row, n[row]:].any()
        assert abs(sc["sum_logprob"][row] - r["sum"]) <= TOKEN_BOUND * r["n"] + abs(r["sum"]) * 2.0 ** -23
        assert abs(sc["avg_logprob"][row] - r["avg"]) <= TOKEN_BOUND + abs(r["avg"]) * 2.0 ** -23


@pytest.mark.parametrize("mode", ["ts", "plain"])
@pytest.mark.parametrize("batch", [5, 32])
def test_every_clip_equals_the_reference_behind_its_own_prompt(engs, mels, ref, mode, batch):
    """5 clips: the cached cross-attention; 32: the absorbed one.  Ids, counts, scores and the no-speech probability."""
    eng, rows = engs[mode], layout(batch)
    ids, n, got = decode(eng, mels[mode], rows)
    whole = 0
    for row, (b, n_ctx) in enumerate(rows):
        r = ref.row(mode, b, n_ctx)
        assert got[row][: r["n0"]] == fed(mode, n_ctx), (row, "the fed prompt")
        if r["first"] is None:
            assert got[row] == r["ids"], (mode, row, b, n_ctx)
            whole += 1
        else:
            assert r["first"] >= 1 and got[row][: r["n0"] + r["first"]] == r["ids"][: r["n0"] + r["first"]], (mode, row, b, n_ctx)
    print(f"{mode} batch {batch}: rows compared whole {whole} of {len(rows)}, generated",
          [len(ref.row(mode, b, c)["ids"]) - ref.row(mode, b, c)["n0"] for b, c in rows[:5]])
    assert whole * 4 >= len(rows) * 3
    check_scores(eng, ref, mode, rows, ids, n)
    assert decode(eng, mels[mode], rows)[2] == got  # again: the same ids
    eng.set_contexts([])
    assert eng.get_option("context_clips") == 0


def test_equal_contexts_are_the_set_context_path(engs, mels):
    eng, mel = engs["ts"], mels["ts"]
    for batch in (5, 32):
        pick = [b % CLIPS for b in range(batch)]
        for n_ctx in (27, 200):
            _, _, got = decode(eng, mel, [(b, n_ctx) for b in pick])
            eng.set_context(context(n_ctx))
            assert eng.get_option("context_clips") == 0  # either kind of context clears the other
            ids, n = eng.encdec_tokens_full(np.ascontiguousarray(mel[pick]))
            assert got == [[int(x) for x in ids[b, : n[b]]] for b in range(batch)], (batch, n_ctx)
            eng.set_context([])


def test_a_clip_in_the_mixed_call_equals_its_call_alone(engs, mels):
    eng, mel = engs["ts"], mels["ts"]
    rows = layout(5)
    ids, n, got = decode(eng, mel, rows)
    lp = eng.last_token_logprobs(ids.shape[1])
    for row, (b, n_ctx) in enumerate(rows):
        ids1, n1, alone = decode(eng, mel, [(b, n_ctx)])
        assert alone[0] == got[row], (row, b, n_ctx)
        lp1 = eng.last_token_logprobs(ids1.shape[1])
        assert np.abs(lp1[0] - lp[row]).max() <= TOKEN_BOUND
    eng.set_contexts([])


def test_sampling_counts_every_clips_own_positions(pkg, models, mels, ref):
    """Temperature 0.6: sample_ref.decode driven with each clip's own prompt — the counter's position word is the id's
    position in the clip's own fed row and its clip word the clip's index, whatever the companions' lengths."""
    milli, seed = 600, 1
    e = cd.new_engine(pkg, models, "ts", scores=1, temperature=milli, seed=seed)
    rows = layout(5)
    ids, n, _ = decode(e, mels["ts"], rows)
    info = e.last_decode_info()
    compared = 0
    for row, (b, n_ctx) in enumerate(rows):
        prompt = fed("ts", n_ctx)
        n0 = len(prompt)
        r = sample_ref.decode(ref.logits_fn("ts", b), prompt, P["ts"], tm.EOT, sm.NOSP, sample_ref.temperature_of_milli(milli), seed,
                              clip=row, beg=tm.BEG, timestamps=True)
        s = sample_ref.first_indecisive(r["infos"], 2 * 1e-4 / (milli / 1000.0))  # the key bar plus twice the logits bar over T
        k = r["n"] if s is None else s
        assert k >= 1 and [int(x) for x in ids[row, : n0 + k]] == r["ids"][: n0 + k], (row, b, n_ctx)
        assert info["temperature_milli"][row] == milli
        compared += k
        if s is None:
            assert n[row] == len(r["ids"])
    print("sampled ids compared:", compared)
    e.close()


def test_graphs_cached_is_unchanged_by_ragged_calls(pkg, models, mels):
    e = cd.new_engine(pkg, models, "ts")
    three = np.ascontiguousarray(mels["ts"][:3])
    plain_ids = e.encdec_tokens_full(three)   # no context: the segment graphs of this call are captured
    held = e.get_option("graphs_cached")
    assert held >= 1
    for lengths in ((0, 1, 2), (5, 0, 63), (27, 27, 3), (0, 0, 0)):
        e.set_contexts([context(k) for k in lengths])
        e.encdec_tokens_full(three)
        assert e.get_option("graphs_cached") == held, lengths
    e.set_contexts([])
    again = e.encdec_tokens_full(three)       # ... and they are still the ones replayed
    assert e.get_option("graphs_cached") == held
    assert np.array_equal(again[0], plain_ids[0]) and np.array_equal(again[1], plain_ids[1])
    e.close()


def test_clearing_the_contexts_restores_the_engine_bit_for_bit(pkg, models, mels):
    three = mels["ts"]
    fresh = cd.new_engine(pkg, models, "ts", scores=1)  # never had a context
    want = (*fresh.encdec_tokens_full(three), fresh.last_scores(), fresh.last_token_logprobs(P["ts"] + 1))
    fresh.close()
    e = cd.new_engine(pkg, models, "ts", scores=1)
    e.set_contexts([context(27), [], context(200)])
    e.encdec_tokens_full(three)
    e.set_contexts([])
    got = (*e.encdec_tokens_full(three), e.last_scores(), e.last_token_logprobs(P["ts"] + 1))
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    e.close()


def test_refusals_leave_the_engine_usable(pkg, models, mels, assets):
    e = cd.new_engine(pkg, models, "ts")
    one, three = np.ascontiguousarray(mels["ts"][:1]), np.ascontiguousarray(mels["ts"][:3])
    want = e.encdec_tokens_full(three)

    def refused(fn, status=UNSUPPORTED, word="context"):
        with pytest.raises(pkg.WtError) as err:
            fn()
        assert status_of(err) == status, str(err.value)
        if word:
            assert word in str(err.value)

    # what set_contexts itself refuses
    refused(lambda: e.set_contexts([[1, 2], [tm.N_VOCAB]]), INVALID)
    refused(lambda: e.set_contexts([[-1]]), INVALID)
    refused(lambda: e.set_contexts([[1]] * 65), INVALID)
    refused(lambda: e.set_contexts([np.zeros(4097, np.int64)]), INVALID)
    assert e.get_option("context_clips") == 0
    e.set_contexts([[1]] * 64)  # the most it takes
    assert e.get_option("context_clips") == 64
    e.set_contexts([context(4), [], context(27)])
    refused(lambda: e.encdec_tokens_full(one), INVALID)   # a batch other than n_clips
    refused(lambda: e.encdec_tokens_full(np.ascontiguousarray(mels["ts"][[0, 1, 2, 0]])), INVALID)
    # a [B][32] call, a pipelined call (both refused with max_positions set, as ever), then calls without max_positions
    refused(lambda: e.encdec_tokens_batch(three), word=None)
    d_mel = DevBuf(three)
    pcm = np.zeros(e.pcm_len, np.float32)
    try:
        refused(lambda: e.pipeline_submit_dev(d_mel.data_ptr(), 3), word=None)
        e.set_option("timestamps", 0)
        e.set_option("max_positions", 0)
        refused(lambda: e.encdec_tokens_batch(three))
        refused(lambda: e.transcribe(pcm))
        refused(lambda: e.pipeline_submit_dev(d_mel.data_ptr(), 3))
    finally:
        d_mel.free()
    e.set_option("max_positions", P["ts"])
    e.set_option("timestamps", 1)
    # beam search, the bf16 storage mode, automatic language: refused by full-length decoding with its own text
    e.set_option("beam_size", 2)
    refused(lambda: e.encdec_tokens_full(three), word=None)
    e.set_option("beam_size", 1)
    e.set_option("bf16", 1)
    refused(lambda: e.encdec_tokens_full(three), word=None)
    e.set_option("bf16", 0)
    language = e.get_option("language")
    e.set_option("language", -1)
    refused(lambda: e.encdec_tokens_full(three), word=None)
    e.set_option("language", language)
    # word timestamps: the alignment pass takes one prompt length per call
    e.set_option("word_timestamps", 1)
    refused(lambda: e.encdec_tokens_full(three), word="word_timestamps")
    e.set_option("word_timestamps", 0)
    # some clip's prompt leaves no position to generate
    e.set_contexts([context(4), [], context(cd.KEEP_TS)])
    e.set_option("max_positions", 1 + cd.KEEP_TS + len(tm.PROMPT))
    refused(lambda: e.encdec_tokens_full(three), INVALID)
    e.set_option("max_positions", 2 + cd.KEEP_TS + len(tm.PROMPT))
    ids, n = e.encdec_tokens_full(three)   # one position left for the longest prompt: it generates one id and is capped
    full = 2 + cd.KEEP_TS + len(tm.PROMPT) + 1
    assert n[2] == (full - 1 if ids[2, full - 2] == tm.EOT else full)
    assert [int(v) for v in ids[2, : full - 2]] == fed("ts", cd.KEEP_TS)
    e.set_option("max_positions", P["ts"])
    e.set_contexts([])
    got = e.encdec_tokens_full(three)      # ... and the engine is as it was
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    e.close()
    # a vocabulary without <|startofprev|>, a Monolith engine
    prefix, vocab = assets("micro")
    m = pkg.Engine(prefix, vocab, True)
    refused(lambda: m.set_contexts([[1, 2, 3]]))
    m.set_contexts([[], []])  # empty contexts all round feed no <|startofprev|>: allowed, as the seeking loop without conditioning needs it
    assert m.get_option("context_clips") == 2
    m.set_contexts([])  # clearing is always allowed
    m.close()
    mono = pkg.Engine(models["ts"][0], models["ts"][1], True, pkg.EngineType.Monolith)
    refused(lambda: mono.set_contexts([[1, 2, 3]]))
    mono.close()
