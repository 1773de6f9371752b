"""The table of tests/mode_schedule.py, checked on the CPU: it is consistent — every option a
kind sets is one reset() restores, every neighbour pair differs in exactly its named setting, every kind passes the
engine's refusal rules — and the neighbour pairs that a CPU reference can decode give DIFFERENT reference results on the
chosen clips.  A stale graph replayed across such a pair is seen by tests/test_gpu_graph_isolation.py only because the
two results differ; the clips, lists and seeds were chosen here, on the CPU oracle, for that."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_full_ref  # noqa: E402
import beam_ref  # noqa: E402
import best_of_ref  # noqa: E402
import mode_schedule as ms  # noqa: E402
import sample_model  # noqa: E402
import sample_ref  # noqa: E402
import suppress_ref  # noqa: E402
import ts_model  # noqa: E402
import ts_ref  # noqa: E402

P = ms.P_SHORT


# ---- the table's consistency ------------------------------------------------------------------------------------------
def test_every_option_a_kind_sets_is_one_reset_restores():
    known = set(ms.DEFAULTS) | set(ms.SPECIAL_DEFAULTS)
    for kind in ms.KINDS.values():
        assert set(kind.options) <= known, kind.name
        assert kind.family in ms.FAMILIES and kind.entry in ms.GETTERS_OF
    assert sorted(ms.FAMILIES) == sorted({k.family for k in ms.KINDS.values()})


def test_reset_writes_every_default_and_clears_the_rest():
    class Recorder:
        def __init__(self):
            self.options, self.calls = {}, {}

        def set_option(self, k, v):
            self.options[k] = v

        def __getattr__(self, name):
            return lambda *a, **kw: self.calls.__setitem__(name, (a, kw))

    r = Recorder()
    ms.reset(r)
    assert r.options == ms.DEFAULTS
    assert r.calls["set_suppress"][0] == ([], []) and r.calls["set_context"][0] == ([],)
    assert r.calls["set_contexts"][0] == ([],) and r.calls["set_prompt"][0] == ([],)
    assert r.calls["set_forced_ids"][0] == (None,) and r.calls["set_alignment_heads"][0] == ((),)
    assert r.calls["dbg_set_alignment"][1] == dict(keep=0, mode=1, sub=0)


def test_every_pair_differs_in_exactly_its_named_setting():
    for a, b, setting in ms.NEIGHBOURS + ms.ARRANGEMENTS:
        ka, kb = ms.KINDS[a], ms.KINDS[b]
        assert ms.differing(ka, kb) == [setting], (a, b)
        assert (ka.entry, ka.clips) == (kb.entry, kb.clips), (a, b)
    named = {s for _, _, s in ms.NEIGHBOURS}
    assert {"max_initial_timestamp", "stop_at_eot", "prompt", "seed", "suppress", "beam_size", "best_of",
            "timestamps"} <= named
    assert {s for _, _, s in ms.ARRANGEMENTS} == {"fc2_ksplit", "cross_chunks", "abs_chunks", "cross_absorb"}
    # the two prompt pairs: other ids at equal length, and another length
    assert len(ms.PROMPT_OTHER_IDS) == len(ms.PROMPT) != len(ms.PROMPT_OTHER_LEN)
    # the two list pairs: equal counts and other ids, and other counts
    assert [len(x) for x in ms.L1] == [len(x) for x in ms.L2] != [len(x) for x in ms.L3] and ms.L1 != ms.L2


def test_every_kind_passes_the_engines_refusal_rules():
    for kind in ms.KINDS.values():
        assert ms.refusal(kind) is None, kind.name
        if kind.entry == "full":
            assert 2 <= len(kind.clips) <= 6 and kind.options["max_positions"] in (ms.P_SHORT, ms.P_LONG)
    # ... and the rules as restated here do refuse what check_full_call / check_beam_call / check_language_call refuse
    full, beam = ms.KINDS["full40/plain"], ms.KINDS["wide/beam2"]
    bad = [
        beam._replace(options=dict(beam.options, context=ms.CONTEXT)),            # no context with full_beam
        beam._replace(options=dict(beam.options, temperature=ms.TEMP)),           # nor a temperature without fallback_beam
        beam._replace(options=dict(beam.options, full_beam=0)),
        full._replace(options=dict(full.options, language=-1)),                   # no language = -1 with max_positions
        full._replace(options=dict(full.options, bf16=1)),
        full._replace(options=dict(full.options, temperature_fallback=1)),        # the fall-back needs scores
        full._replace(options=dict(full.options, word_timestamps=1)),             # word_timestamps needs timestamps
        full._replace(options=dict(full.options, contexts=((1,), (2,), (3,)))),   # another number of clips
        ms.KINDS["wide/best_of3"]._replace(options=dict(ms.KINDS["wide/best_of3"].options, stop_at_eot=0)),
        ms.KINDS["short/beam2"]._replace(options=dict(beam_size=2, stop_at_eot=0)),
        ms.KINDS["short/beam2"]._replace(options=dict(beam_size=2, language=-1)),
        ms.KINDS["short/default"]._replace(options=dict(timestamps=1)),           # full-length decoding only
        ms.KINDS["short/language_auto"]._replace(options=dict(language=-1, prompt=tuple(ms.PROMPT))),
    ]
    for kind in bad:
        assert ms.refusal(kind) is not None, kind.options


def test_key_families_of_the_kinds():
    """Which graph keys a kind's chains take: the five families are all in the table, and calls with a context take none."""
    seen = set()
    for kind in ms.KINDS.values():
        seen |= set(ms.key_families(kind))
    assert seen == {"greedy", "beam", "full", "beam_full", "best_of"}
    assert ms.key_families(ms.KINDS["full40/context"]) == () == ms.key_families(ms.KINDS["full96/contexts"])
    assert ms.key_families(ms.KINDS["wide/best_of3"]) == ("best_of",)
    assert ms.key_families(ms.KINDS["wide/fallback_beam"]) == ("beam_full", "best_of")
    assert ms.key_families(ms.KINDS["full40/fallback"]) == ("full",)
    assert [k.name for k in ms.KINDS.values() if ms.per_slot(k)] == ["short/beam2", "short/beam4"]


# ---- the neighbour pairs on the CPU references ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref(pkg, orc, assets, tmp_path_factory):
    prefix, _ = assets("micro")
    path = str(tmp_path_factory.mktemp("mode-schedule") / "micro-schedule.wtw")
    ms.write_model(prefix + ".wtw", path)
    model = orc.Model(path)
    data = ms.Data()
    enc = {b: model.encode(data.mel[b]) for b in ms.C2}
    yield model, enc
    model.close()


def greedy(ref, b, prompt, max_pos, stop_at_eot=True):
    model, enc = ref
    ids, _ = model.decode_greedy(enc[b], prompt, max_pos, ms.EOT, stop_at_eot)
    return [int(i) for i in ids]


def test_stop_at_eot_pairs_a_clip_reaches_eot_early(ref):
    """short/default against short/no_eot, full40/plain against full40/no_eot: some clip emits EOT before the last
    position, and the decode that goes on behind it differs from the one that stops."""
    for max_pos in (30, P):
        early = [b for b in ms.C2 if greedy(ref, b, ms.PROMPT, max_pos)[-1] == ms.EOT and len(greedy(ref, b, ms.PROMPT, max_pos)) < max_pos]
        assert early, max_pos
        for b in early:
            assert len(greedy(ref, b, ms.PROMPT, max_pos, False)) == max_pos + 1 > len(greedy(ref, b, ms.PROMPT, max_pos))


def test_prompt_pairs_differ(ref):
    base = [greedy(ref, b, ms.PROMPT, 30)[len(ms.PROMPT):] for b in ms.C2]
    other_ids = [greedy(ref, b, ms.PROMPT_OTHER_IDS, 30)[len(ms.PROMPT):] for b in ms.C2]
    other_len = [greedy(ref, b, ms.PROMPT_OTHER_LEN, 30)[len(ms.PROMPT_OTHER_LEN):] for b in ms.C2]
    assert other_ids != base                 # the generated ids, not the prompts alone
    assert other_len != base


def test_max_tokens_pair_differs(ref):
    assert any(len(greedy(ref, b, ms.PROMPT, 30)) > 12 for b in ms.C2)   # max_tokens = 12 cuts a row short


def ts_rows(ref, max_initial):
    model, enc = ref
    return [ts_ref.decode(ts_model.logits_fn(model, enc[b], P), ms.PROMPT_TS, P, ms.EOT, ms.BEG, max_initial)[0] for b in ms.C2]


def test_max_initial_timestamp_and_timestamps_pairs_differ(ref):
    a, z = ts_rows(ref, 50), ts_rows(ref, ms.MAX_INITIAL_OTHER)
    n = len(ms.PROMPT_TS)
    for ra, rz in zip(a, z):
        assert ra[n] != rz[n] == ms.BEG           # the first generated id is the rule's own
        assert ms.BEG < ra[n] <= ms.BEG + 50
    assert any(ra[n + 1:] != rz[n + 1:] for ra, rz in zip(a, z))   # ... and a clip goes another way behind it
    plain = [greedy(ref, b, ms.PROMPT, P)[len(ms.PROMPT):] for b in ms.C2]
    assert all(r[n:] != p for r, p in zip(a, plain))                # with against without timestamps


def test_suppression_list_pairs_differ(ref):
    model, enc = ref

    def rows(lists):
        return [suppress_ref.greedy(ts_model.logits_fn(model, enc[b], P), ms.PROMPT, P, ms.EOT, lists[0], lists[1])[0] for b in ms.C2]

    plain, l1, l2, l3 = rows(((), ())), rows(ms.L1), rows(ms.L2), rows(ms.L3)
    assert all(a != b for a, b in zip(plain, l1))
    assert all(a != b for a, b in zip(l1, l2))
    assert all(a != b for a, b in zip(l1, l3))


def sampled(ref, seed, word=0):
    model, enc = ref
    return [sample_ref.decode(sample_model.logits_fn(model, enc[b]), ms.PROMPT, P, ms.EOT, ms.NOSP,
                              sample_ref.temperature_of_milli(ms.TEMP), seed, c, word, ms.BEG, False) for c, b in enumerate(ms.C2)]


def test_seed_and_best_of_pairs_differ(ref):
    a, b = sampled(ref, ms.SEED_A), sampled(ref, ms.SEED_B)
    assert all(x["ids"] != y["ids"] for x, y in zip(a, b))
    # best_of = 3 under SEED_A: the kept sample is not the one best_of = 1 draws, on every clip
    words = [best_of_ref.attempt_word(0, j) for j in range(3)]
    samples = [a] + [sampled(ref, ms.SEED_A, w) for w in words[1:]]
    for c in range(len(ms.C2)):
        picked = best_of_ref.rank([s[c]["sum"] for s in samples], [s[c]["n"] for s in samples])
        assert picked != 0 and samples[picked][c]["ids"] != a[c]["ids"], c


def test_beam_size_pairs_differ(ref):
    model, enc = ref
    full, short = {}, {}
    for b in ms.C2:
        fn = beam_full_ref.level_logits_fn(model, enc[b], ms.EOT)
        full[b] = [beam_full_ref.beam_search(fn, ms.PROMPT, K, P, ms.EOT)["ids"] for K in (2, 3)]
        fn = beam_ref.oracle_logits_fn(model, enc[b], ms.EOT)
        short[b] = [beam_ref.beam_search(fn, ms.PROMPT, K, 30, ms.EOT)["ids"] for K in (2, 4)]
    assert any(full[b][0] != full[b][1] for b in ms.C2)      # wide/beam2 against wide/beam3
    assert any(short[b][0] != short[b][1] for b in ms.C2)    # short/beam2 against short/beam4
