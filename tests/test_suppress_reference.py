"""Logit suppression on the CPU: the reference filter of tests/suppress_ref.py on hand-made rows,
in front of the references it composes with; the pins of the fixtures and lists tests/test_gpu_suppress.py decodes
(tests/suppress_model.py) over the CPU oracle; and wt_vocab_default_suppress against its Python restatement on synthetic
vocabularies.  The hand-made rows and the pins run the reference and the oracle alone, as reference pins do; the
default-list cases call wt_vocab_default_suppress, which does not exist without the feature.  CPU only."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_full_ref as bfr  # noqa: E402
import full_model as fm  # noqa: E402
import sample_ref  # noqa: E402
import scores_model as sm  # noqa: E402
import scores_ref  # noqa: E402
import suppress_model as spm  # noqa: E402
import suppress_ref as sup  # noqa: E402
import ts_ref  # noqa: E402

N_TS, N_PLAIN = len(sm.TS_PROMPT), len(sm.PLAIN_PROMPT)


# ---- hand-made rows ---------------------------------------------------------------------------------------------------

def table_fn(rows):
    """A logits function over a table: the row of a prefix is picked by its length."""
    return lambda prefix: np.asarray(rows[len(prefix)], np.float32)


def test_a_listed_argmax_is_not_chosen():
    z = np.array([0.0, 3.0, 2.0, 1.0], np.float32)
    assert int(np.argmax(z)) == 1
    ids, margins = sup.greedy(table_fn({1: z, 2: z}), [9], 2, eot=3, ids=[1])
    assert ids == [9, 2, 2] and np.allclose(margins, [1.0, 1.0])
    assert np.array_equal(sup.filter_row(z, 5, [1]), np.array([0.0, -np.inf, 2.0, 1.0], np.float32))
    assert z[1] == 3.0  # a copy: the caller's row is untouched


def test_the_first_list_holds_at_the_first_position_only():
    z = np.array([0.0, 3.0, 2.0, 1.0], np.float32)
    ids, _ = sup.greedy(table_fn({2: z, 3: z}), [9, 9], 3, eot=0, first_ids=[1])
    assert ids == [9, 9, 2, 1]  # n_gen = 0: masked; n_gen = 1: allowed
    fn = sup.wrap(table_fn({1: z, 2: z, 3: z}), 2, [], [1])
    assert fn([9])[1] == 3.0 and fn([9, 9])[1] == -np.inf and fn([9, 9, 2])[1] == 3.0  # a prompt position is not generated


def test_the_filter_comes_before_the_log_softmax():
    rng = np.random.default_rng(0)
    z = rng.standard_normal(50).astype(np.float32) * 3
    tok = int(np.argsort(z)[-3])
    listed = [int(i) for i in np.argsort(z)[-2:]]
    lp0, _ = scores_ref.token_logprob(z, tok)
    lp1, _ = scores_ref.token_logprob(sup.filter_row(z, 1, listed), tok)
    p = float(np.exp(z[listed].astype(np.float64) - scores_ref.logsumexp64(z)).sum())
    assert p > 0.3 and abs((lp1 - lp0) + math.log1p(-p)) < 1e-12


def test_rule_5_flips_when_the_best_text_id_is_listed():
    eot, beg, V = 10, 12, 20
    z = np.full(V, -5.0, np.float32)
    z[3], z[4] = 4.0, 2.0              # the best text id and the runner-up
    z[beg + 3:beg + 8] = 1.5           # five timestamps: logsumexp = 1.5 + log 5 = 3.1
    g = [beg + 1, 5]
    tok, info = ts_ref.step(z, g, eot, beg)
    assert tok == 3 and "mass" not in info["fired"]
    tok, info = ts_ref.step(sup.filter_row(z, len(g), [3]), g, eot, beg)
    assert tok >= beg and "mass" in info["fired"] and "mass_decided" in info["fired"]


def test_a_beam_hypothesis_with_fewer_than_k_plus_one_allowed_ids():
    eot, K = 5, 3
    z = np.array([1.0, 2.0, 3.0, 4.0, 0.5, 0.0], np.float32)
    lp, _ = bfr.step_lp(sup.filter_row(z, 1, [0, 1, 2]), [1], eot)
    assert len(bfr.offered(lp, K)) == 3 < K + 1
    table = {n: z for n in range(1, 8)}
    r = bfr.beam_search(sup.wrap(table_fn(table), 1, [0, 1, 2]), [7], K, 4, eot)
    plain = bfr.beam_search(table_fn(table), [7], K, 4, eot)
    # the first hypothesis offers ids 3 and 4 and EOT: two live ones enter the next step, not K
    assert r["n_live"][:2] == [1, 2] and plain["n_live"][:2] == [1, K] and not set(r["ids"][1:]) & {0, 1, 2}


def test_sampling_never_draws_a_listed_id():
    z = np.zeros(8, np.float32)
    z[2] = 9.0
    drawn = {sample_ref.step(sup.filter_row(z, 1, [2]), [0], 1.0, seed=s, pos=4)[0] for s in range(40)}
    assert 2 not in drawn and len(drawn) >= 4
    assert {sample_ref.step(z, [0], 1.0, seed=s, pos=4)[0] for s in range(40)} == {2}


# ---- the fixtures the GPU tests decode -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref(orc, assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    r = spm.Reference(orc, spm.write_models(prefix, vocab, str(tmp_path_factory.mktemp("suppress-ref"))), spm.all_mels())
    yield r
    r.close()


def within_cap(rows):
    """At most one clip in six is set aside as indecisive: in a case of fewer than six clips, none."""
    aside = [b for b, r in enumerate(rows) if r["first"] is not None]
    assert len(aside) <= len(rows) // spm.ASIDE_CAP, aside


def greedy_margins(rows):
    """Every compared step's top-two margin over the allowed set (and rule 5's gap) exceeds fm.MARGIN."""
    for r in rows:
        steps = r["infos"] if r["first"] is None else r["infos"][: r["first"]]
        assert all(min(i["gap"], i["gap_lm"]) > fm.MARGIN for i in steps)


def pins(ref, mode, clips, P, n0, lists_P=None, prompt=None, V=51865, **kw):
    lists = ref.lists_of(mode, clips, P if lists_P is None else lists_P, prompt=prompt, V=V)
    plain = [ref.row(mode, b, P, prompt=prompt) for b in clips]
    want = [ref.row(mode, b, P, lists, prompt=prompt, **kw) for b in clips]
    spm.check_rows([r["ids"] for r in want], [r["ids"] for r in plain], n0, *lists)
    within_cap(want)
    greedy_margins(want)
    return lists, plain, want


def test_pins_plain_greedy_on_the_eot_rich_model(ref):
    lists, plain, want = pins(ref, "rich", spm.RICH_CLIPS, spm.P_GREEDY, N_PLAIN)
    assert lists == ([0, 16, 51864], [16, fm.EOT])
    assert min(min(i["gap"] for i in r["infos"]) for r in want) > fm.MARGIN
    assert any(len(p["ids"]) < spm.P_GREEDY + 1 for p in plain) and any(len(r["ids"]) > 33 for r in want)
    # the lists of equal counts test_gpu_suppress.py swaps in between two calls give other ids
    other = spm.other_lists(lists, want[0], N_PLAIN)
    assert other[0] != lists[0] and len(other[0]) == len(lists[0]) and other[1] == lists[1]
    rows = [ref.row("rich", b, spm.P_GREEDY, other) for b in spm.RICH_CLIPS[:2]]
    assert all(r["first"] is None for r in rows) and [r["ids"] for r in rows] != [r["ids"] for r in want[:2]]


def test_pins_clips_that_opened_with_eot(ref):
    lists, plain, want = pins(ref, "first", spm.FIRST_CLIPS, spm.P_SHORT, N_PLAIN)
    assert fm.EOT in lists[1] and sm.NOSP in lists[1]  # <|nospeech|> itself opens clips of the unfiltered decode
    opened = [b for b, r in enumerate(plain) if r["ids"][N_PLAIN] == fm.EOT]
    assert len(opened) >= 2 and all(len(want[b]["ids"]) > N_PLAIN + 1 for b in opened)
    assert all(r["first"] is None for r in want)
    assert [r["no_speech_prob"] for r in want] == [r["no_speech_prob"] for r in plain]  # read from the unfiltered logits


def test_pins_timestamps_and_scores(ref):
    lists, plain, want = pins(ref, "ts", spm.TS_CLIPS, spm.P_TS, N_TS)
    assert all(r["first"] is None for r in want)
    assert all(r["ids"][N_TS] >= sm.BEG for r in want)  # rule 4 still holds behind the filter
    assert lists[0][-1] == 51864 and all(i >= sm.BEG for i in lists[1] if i != sm.EOT)


def test_pins_sampling(ref):
    lists = ref.lists_of("ts", spm.TS_CLIPS, spm.P_TS)
    rows = [ref.row("ts", b, spm.P_SHORT, lists, milli=600, seed=1, rng_clip=i) for i, b in enumerate(spm.TS_CLIPS)]
    greedy = [ref.row("ts", b, spm.P_SHORT, lists) for b in spm.TS_CLIPS]
    assert [r["ids"] for r in rows] != [r["ids"] for r in greedy]
    within_cap(rows)
    for r in rows:
        assert not set(r["ids"][N_TS:]) & set(lists[0]) and r["ids"][N_TS] not in lists[1]


@pytest.mark.parametrize("K", [2, 5])
def test_pins_beam_sums_stay_apart(ref, K):
    lists = ref.lists_of("ts", spm.TS_CLIPS, spm.P_TS)
    aside = 0
    for b in spm.TS_CLIPS:
        fn = sup.wrap(ref.raw("ts", b, spm.P_SHORT, lookahead=False), N_TS, *lists)
        r = bfr.beam_search(fn, sm.TS_PROMPT, K, spm.P_SHORT, sm.EOT, sm.BEG, True)
        assert not set(r["ids"][N_TS:]) & set(lists[0]) and r["ids"][N_TS] not in lists[1]
        aside += r["margin"] <= spm.DELTA  # beam sums apart by more than delta
    assert aside <= len(spm.TS_CLIPS) // spm.ASIDE_CAP


def test_pins_a_context(ref):
    lists = ref.lists_of("first", spm.FIRST_CLIPS, spm.P_SHORT)
    ctx = spm.context(spm.CONTEXT_IDS)
    plain = [ref.row("first", b, spm.P_CTX, ((), ()), ctx) for b in (0, 1, 2)]
    want = [ref.row("first", b, spm.P_CTX, lists, ctx) for b in (0, 1, 2)]
    assert any(p["ids"][p["n0"]] in lists[1] for p in plain)
    assert all(r["ids"][r["n0"]] not in lists[1] and r["n0"] == spm.CONTEXT_IDS + 1 + N_PLAIN for r in want)
    within_cap(want)
    greedy_margins(want)
    ragged = [ref.row("first", b, spm.P_CTX, lists, c) for b, c in zip((0, 1, 2), ([], spm.context(5, 1), ctx))]
    within_cap(ragged)
    greedy_margins(ragged)


def test_pins_fallback(ref):
    """Every attempt of every clip of the fall-back case is decisive, so the accept decisions are the reference's."""
    import sample_model as smp
    lists = ref.lists_of("ts", spm.TS_CLIPS, spm.P_TS)
    fb = smp.FB
    temps = sample_ref.schedule(fb["temperature"], fb["temperature_increment"])
    for i, b in enumerate(spm.TS_CLIPS):
        within_cap([ref.row("ts", b, spm.P_SHORT, lists, milli=t, seed=fb["seed"], rng_clip=i, attempt=a)
                    for a, t in enumerate(temps)])


# ---- the default lists -------------------------------------------------------------------------------------------------

def write_vocab(pkg, path, tokens):
    """A vocabulary file of the given tokens (bytes) behind the synthetic file's filter bank."""
    import struct
    src = path + ".src"
    pkg.write_synthetic_vocab(src, 1)
    raw = open(src, "rb").read()
    n_mel, n_fft = struct.unpack_from("<ii", raw, 12)
    head = raw[8: 8 + 12 + 4 * n_mel * n_fft]
    body = struct.pack("<i", len(tokens)) + b"".join(struct.pack("<I", len(t)) + t for t in tokens)
    payload = head + body
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(payload)) + payload)


def tokens_with(extra, n=300):
    toks = [bytes([65 + i % 26]) * (2 + i // 26) for i in range(n)]  # words of letters: none is a symbol
    for i, t in extra.items():
        toks[i] = t
    return toks


NOTE = "♫".encode()  # e2 99 ab


@pytest.mark.parametrize("case", ["full", "no_blank", "multilingual"])
def test_default_lists_equal_the_restatement(pkg, tmp_path, case):
    extra = {7: b" ", 9: b"-", 11: b" -", 13: "♪".encode(), 15: NOTE[:2], 17: NOTE[:1], 19: b"(", 21: b" (", 23: b"--",
             25: " ♪♪".encode(), 27: b" " + NOTE[:2], 29: b"(", 31: b"'"}
    if case == "no_blank":
        del extra[7]
    path = str(tmp_path / "vocab.bin")
    write_vocab(pkg, path, tokens_with(extra))
    v = pkg.Vocab(path, case == "multilingual")
    info = v.info()
    tokens = {i: v.token(i) for i in range(300)}
    ids, first = v.default_suppress()
    want_ids, want_first = sup.default_lists(tokens, info)
    assert list(ids) == want_ids and list(first) == want_first
    assert list(ids) == sorted(set(ids)) and list(first) == sorted(set(first))
    # exact matches of s and " " + s, the exact " -"; "-" alone and "'" alone are no symbols of the list
    assert {11, 13, 19, 21, 23} <= set(ids) and 9 not in ids and 31 not in ids and 29 not in ids
    # the two-byte prefix token of ♫ stands in for the symbol (the longest, not the one-byte one), also behind a space
    assert 15 in ids and 17 not in ids and 27 in ids
    assert 7 not in ids  # the bare space is never on the always-list
    if case == "multilingual":  # n_vocab = 51865: the special ids and EOT exist
        assert {info[k] for k in ("sot", "prev", "solm", "translate", "transcribe")} <= set(ids)
        # Whisper's six: sot, translate, transcribe, startoflm, startofprev, nospeech
        assert [i for i in ids if i >= 300] == [50258, 50358, 50359, 50360, 50361, 50362]
        assert list(first) == [7, info["eot"]] and info["eot"] not in ids
    else:  # a vocabulary that ends before sot: no special id, no EOT
        assert info["n_vocab"] == 300 and max(ids) < 300
        assert list(first) == ([7] if case == "full" else [])
    # buffers too small: the counts still come back
    import ctypes
    n, nf = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = pkg.lib().wt_vocab_default_suppress(v._v, None, 0, ctypes.byref(n), None, 0, ctypes.byref(nf))
    assert pkg.STATUS_NAMES[rc] == ("WT_ERR_BUFFER" if len(ids) + len(first) else "WT_OK")
    assert (n.value, nf.value) == (len(ids), len(first))
    v.close()
