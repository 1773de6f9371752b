"""The rules of full-length beam search (tests/beam_full_ref.py) on hand-made tables, and the pins
of the fixtures tests/ts_model.py and tests/full_model.py under them on the CPU oracle, so that
tests/test_gpu_beam_full.py cannot pass vacuously.  Every search is computed once per module.  CPU only."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_full_ref as bfr  # noqa: E402
import full_model as fm  # noqa: E402
import ts_model as tm  # noqa: E402
import ts_ref  # noqa: E402

DELTA = 2e-4  # the decisive-margin rule of tests/test_gpu_beam_full.py
# a small vocabulary: text 0..5, eot 6, specials 7..9, timestamps 10..19 (ticks 0..9)
V, EOT, BEG = 20, 6, 10


def table(**at):
    z = np.full(V, -5.0, np.float32)
    for k, v in at.items():
        z[int(k[1:])] = v
    return z


def lse(values):
    v = np.asarray(values, np.float64)
    return float(v.max() + math.log(np.exp(v - v.max()).sum()))


def test_filter_first_then_log_softmax():
    z = table(i2=1.0, i8=9.0, i12=0.5)
    lp, gap = bfr.step_lp(z, [BEG + 1, 3], EOT, BEG, True)  # text, EOT and ticks >= 2 are allowed; the specials are not
    allowed = [i for i in range(V) if i <= EOT or i >= BEG + 2]
    assert [i for i in range(V) if lp[i] != -np.inf] == allowed
    assert lp[2] == pytest.approx(1.0 - lse(z[allowed])) and gap == pytest.approx(abs(lse(z[BEG + 2:]) - 1.0))
    plain, gap = bfr.step_lp(z, [BEG + 1, 3], EOT)  # without timestamps A is the whole vocabulary
    assert plain[8] == pytest.approx(9.0 - lse(z)) and gap == math.inf
    z[BEG + 2:] = 3.0  # rule 5: log(8) + 3 > 1, the text ids leave A
    lp, _ = bfr.step_lp(z, [BEG + 1, 3], EOT, BEG, True)
    assert [i for i in range(V) if lp[i] != -np.inf] == list(range(BEG + 2, V))
    assert lp[BEG + 2] == pytest.approx(-math.log(8.0))
    z[4] = -np.inf  # a logit of -inf is a masked id
    assert bfr.step_lp(z, [], EOT)[0][4] == -np.inf


def test_k1_is_the_filtered_greedy_decode():
    def fn(prefix):
        n = len(prefix) - 2
        return table(i2=3.0, i12=2.0) if n < 4 else table(i6=9.0)
    for P in (20, 4):
        want, _ = ts_ref.decode(fn, [7, 8], P, EOT, BEG)
        assert bfr.beam_search(fn, [7, 8], 1, P, EOT, BEG, True)["ids"] == want
    z = table(i1=2.0, i3=2.0, i6=0.0)  # and of the plain one without timestamps: ties take the larger id
    assert bfr.beam_search(lambda p: z if len(p) < 5 else table(i6=9.0), [7, 8], 1, 12, EOT)["ids"] == [7, 8, 3, 3, 3, EOT]


def test_a_smaller_than_k_plus_1_leaves_fewer_live_hypotheses():
    """max_initial = 1: the first step offers 2 ids, so 2 hypotheses are live at K = 4; the next step restores 4."""
    def fn(prefix):
        g = prefix[2:]
        if not g:
            return table(i10=1.0, i11=0.5, i12=9.0)
        return table(i1=2.0, i2=1.5, i3=1.0, i4=0.5, i6=-1.0)
    r = bfr.beam_search(fn, [7, 8], 4, 6, EOT, BEG, True, 1)
    assert r["n_live"][:3] == [1, 2, 4]
    assert r["ids"][2] == BEG  # tick 2 is past max_initial however loud it is
    one = bfr.beam_search(fn, [7, 8], 4, 6, EOT, BEG, True, 0)
    assert one["n_live"][:3] == [1, 1, 4]


def test_a_clip_may_end_with_no_live_hypothesis():
    """The first step's A holds two ids and every id but EOT is masked afterwards: both candidates finish, nothing stays
    live, and the clip ends with fewer than K = 4 finished hypotheses."""
    def fn(prefix):
        z = np.full(V, -np.inf, np.float32)
        if len(prefix) == 2:
            z[1], z[2] = 2.0, 1.0
        else:
            z[EOT] = 0.0
        return z
    r = bfr.beam_search(fn, [7, 8], 4, 10, EOT)
    assert r["n_live"] == [1, 2] and not r["done_early"]  # (done_early: K finished)
    assert [g for g, _ in r["finished"]] == [[1, EOT], [2, EOT]] and r["ids"] == [7, 8, 1, EOT]
    assert r["sum"] == pytest.approx(2.0 - lse([2.0, 1.0]))  # the EOT step's lp is 0: A holds one id
    r = bfr.beam_search(fn, [7, 8], 2, 10, EOT)  # K = 2: the same two finish, and that is K
    assert r["n_live"] == [1, 2] and r["done_early"] and len(r["finished"]) == 2


def test_siblings_with_different_histories_get_different_allowed_sets():
    """One hypothesis ends in text behind a timestamp, its sibling in one timestamp behind text: the same logits give
    them different A, and different lp for the same id."""
    def fn(prefix):
        g = prefix[2:]
        if not g:
            return table(i10=1.0)
        if len(g) == 1:
            return table(i2=1.0)   # after [ts]: pen_ts holds, text follows
        if len(g) == 2:
            return table(i3=2.0, i12=1.9)  # [ts, text]: text or a later timestamp
        return table(i4=1.0, i15=0.9, i6=0.0)
    r = bfr.beam_search(fn, [7, 8], 2, 6, EOT, BEG, True, 0)
    hyp_text, hyp_stamp = [BEG, 2, 3], [BEG, 2, BEG + 2]
    z = fn([7, 8] + hyp_text)
    lp_text, _ = bfr.step_lp(z, hyp_text, EOT, BEG, True, 0)
    lp_stamp, _ = bfr.step_lp(z, hyp_stamp, EOT, BEG, True, 0)
    assert lp_text[15] > -np.inf and lp_text[4] > -np.inf     # text behind a timestamp: both classes
    assert lp_stamp[4] == -np.inf and lp_stamp[15] > -np.inf  # text, then one timestamp: text is forbidden
    assert lp_stamp[15] > lp_text[15]
    assert r["n_live"][:4] == [1, 1, 2, 2]  # max_initial 0: one id at the first step, so one hypothesis at the second


def test_the_search_to_a_shorter_cap_is_the_longer_one_stopped_there():
    def fn(prefix):
        n = len(prefix) - 2
        return table(i2=3.0, i3=2.9, i12=2.0, i6=1.0 + 0.4 * n)
    both = bfr.beam_search(fn, [7, 8], 3, (12, 5), EOT, BEG, True)
    for P in (12, 5):
        assert both[P] == bfr.beam_search(fn, [7, 8], 3, P, EOT, BEG, True)
    assert both[12]["ids"] != both[5]["ids"]


def test_lps_are_the_teacher_forced_ones():
    def fn(prefix):
        rng = np.random.default_rng(len(prefix) * 7 + int(sum(prefix)))
        return (3.0 * rng.standard_normal(V)).astype(np.float32)
    r = bfr.beam_search(fn, [7, 8], 3, 12, EOT, BEG, True)
    lps, total = bfr.teacher_forced(fn, r["ids"], 2, EOT, BEG, True)
    assert lps == pytest.approx(r["lps"], abs=1e-12) and total == pytest.approx(r["sum"], abs=1e-12)
    assert r["n_gen"] == len(r["ids"]) - 2 == len(r["lps"])


# ----------------------------------------------------------- the fixtures ---

def searches(model, mel, prompt, Ks, caps, timestamps, mit=50):
    """{(K, P): the clips' results}: one search per (clip, K) serves both caps."""
    out = {}
    for K in Ks:
        rows = [bfr.beam_search(bfr.level_logits_fn(model, model.encode(mel[b]), tm.EOT), prompt, K, caps, tm.EOT, tm.BEG,
                                timestamps, mit) for b in range(mel.shape[0])]
        for P in caps:
            out[(K, P)] = [r[P] for r in rows]
    return out


def indecisive(rows):
    return [b for b, r in enumerate(rows) if not r["margin"] > DELTA]


@pytest.fixture(scope="module")
def ts_model(orc, assets, tmp_path_factory):
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("beamfull") / "micro-ts.wtw")
    tm.write_model(prefix + ".wtw", p)
    model = orc.Model(p)
    yield model
    model.close()


@pytest.fixture(scope="module")
def ts_rows(ts_model):
    return searches(ts_model, tm.mels(), tm.PROMPT, (1, 2, 4, 5), (tm.P_LONG, tm.P_SHORT), True)


def test_ts_fixture_k1_is_ts_ref_decode(ts_model, ts_rows):
    greedy = tm.reference_rows(ts_model, tm.mels(), tm.P_LONG)
    for P in (tm.P_LONG, tm.P_SHORT):
        want = tm.cut_rows(greedy, P)
        assert [r["ids"] for r in ts_rows[(1, P)]] == [ids for ids, _ in want]


def test_ts_fixture_is_decisive_and_differs_from_greedy(ts_rows):
    smallest = math.inf
    for K in (2, 4, 5):
        for P in (tm.P_LONG, tm.P_SHORT):
            rows = ts_rows[(K, P)]
            print(f"K {K} P {P}: margins", ["%.1e" % r["margin"] for r in rows], "ids", [len(r["ids"]) for r in rows])
            assert len(indecisive(rows)) * 4 <= len(rows)
            assert not indecisive(rows)  # the fixture as chosen: every clip
            smallest = min(smallest, min(r["margin"] for r in rows))
        assert all(r["done_early"] for r in ts_rows[(K, tm.P_LONG)])  # K hypotheses finish before the cap
        assert not all(r["done_early"] for r in ts_rows[(K, tm.P_SHORT)])
        assert [r["ids"] for r in ts_rows[(K, tm.P_LONG)]] != [r["ids"] for r in ts_rows[(1, tm.P_LONG)]]
    assert 3e-4 < smallest < 5e-4  # 3.5e-4, at K = 5 and P = 96
    assert len(ts_rows[(5, tm.P_LONG)][0]["ids"]) == 38 and len(ts_rows[(1, tm.P_LONG)][0]["ids"]) == tm.P_LONG + 1
    for rows in ts_rows.values():  # the rules hold on every result
        for r in rows:
            gen = r["ids"][len(tm.PROMPT):]
            stamps = [i for i in gen if i >= tm.BEG]
            assert tm.BEG <= gen[0] <= tm.BEG + 50 and stamps == sorted(stamps)
            assert not any(tm.EOT < i < tm.BEG for i in gen)


@pytest.mark.parametrize("mit,live,set_aside", [(2, 3, 0), (0, 1, 1)])
def test_ts_fixture_max_initial_timestamp(ts_model, mit, live, set_aside):
    rows = searches(ts_model, tm.mels(), tm.PROMPT, (4,), (tm.P_SHORT,), True, mit)[(4, tm.P_SHORT)]
    print(f"max_initial {mit}: margins", ["%.2e" % r["margin"] for r in rows])
    assert all(r["n_live"][:2] == [1, live] for r in rows)  # the first step offers mit + 1 ids
    assert all(tm.BEG <= r["ids"][len(tm.PROMPT)] <= tm.BEG + mit for r in rows)
    # (at max_initial 0 one clip sits at the margin itself and is set aside)
    assert len(indecisive(rows)) == set_aside and len(indecisive(rows)) * 4 <= len(rows)


def test_eot_rich_fixture_without_timestamps(orc, assets, tmp_path_factory):
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("beamfull") / "micro-rich.wtw")
    fm.write_eot_rich(prefix + ".wtw", p)
    model = orc.Model(p)
    mel = fm.mels(fm.RICH_CLIPS, (80, 200), fm.RICH_SEED)
    rows = searches(model, mel, fm.RICH_PROMPT, (2, 4), (160, 40), False)
    model.close()
    smallest, slots = math.inf, set()
    for key, rs in rows.items():
        print(key, "margins", ["%.1e" % r["margin"] for r in rs], "ids", [len(r["ids"]) for r in rs])
        assert not indecisive(rs)
        smallest = min(smallest, min(r["margin"] for r in rs))
        slots |= {s for r in rs for s in r["eot_slots"]}
    assert 3e-4 < smallest < 5e-4  # 3.8e-4
    assert slots == {0, 1}  # accepted EOTs come from more than one slot
    lens = [len(r["ids"]) for r in rows[(4, 160)]]
    assert min(lens) < 32 and max(lens) > 64  # ends inside the first segment and past the second
