"""The timestamp rules and the segment parser of tests/ts_ref.py on hand-made tables, wt_vocab_segments against the
Python parser, and the pins of the fixture tests/ts_model.py on the CPU oracle (option timestamps, DESIGN.md section
14), so that tests/test_gpu_timestamps.py cannot pass vacuously.  CPU only."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ts_model as tm  # noqa: E402
import ts_ref  # noqa: E402

# a small vocabulary: text 0..5, eot 6, specials 7..9, timestamps 10..19 (ticks 0..9)
V, EOT, BEG = 20, 6, 10


def table(**at):
    z = np.full(V, -5.0, np.float32)
    for k, v in at.items():
        z[int(k[1:])] = v
    return z


def test_rule1_specials_are_never_chosen():
    z = table(i8=9.0, i3=1.0)
    tok, info = ts_ref.step(z, [BEG + 1, 2], EOT, BEG)
    assert tok == 3 and info["plain"] == 8


def test_rule2_text_follows_a_pair_and_a_pair_follows_text():
    z = table(i15=9.0, i2=1.0)
    tok, info = ts_ref.step(z, [BEG + 1], EOT, BEG)  # |g| = 1: pen_ts holds, the opening timestamp counts as a pair
    assert tok == 2 and "text_after_pair" in info["fired"] and info["L"] is None
    tok, info = ts_ref.step(z, [BEG + 1, 3, BEG + 4, BEG + 4], EOT, BEG)
    assert tok == 2 and "text_after_pair" in info["fired"]
    z = table(i2=9.0, i15=1.0)
    tok, info = ts_ref.step(z, [BEG + 1, 3, BEG + 4], EOT, BEG)  # text, then ONE timestamp: text is forbidden
    assert tok == BEG + 5 and "text_forbidden" in info["fired"]
    z = table(i2=9.0, i6=8.0, i15=1.0)
    tok, info = ts_ref.step(z, [BEG + 1, 3, BEG + 4], EOT, BEG)  # ... EOT is not
    assert tok == EOT and info["M"] == 8.0


def test_rule3_timestamps_never_decrease():
    z = table(i12=9.0, i14=3.0, i15=2.0, i1=0.0)
    tok, info = ts_ref.step(z, [BEG + 1, 3, BEG + 4], EOT, BEG)  # closing side: the same tick may repeat
    assert tok == BEG + 4 and {"monotonic", "monotonic_decided"} <= info["fired"]
    tok, info = ts_ref.step(z, [BEG + 1, 3, BEG + 4, BEG + 4, 2], EOT, BEG)  # after text: strictly later
    assert tok == BEG + 5 and "monotonic_decided" in info["fired"]
    tok, info = ts_ref.step(table(i1=1.0), [BEG + 9, 3], EOT, BEG)  # tick 9 of 9 reached: no timestamp is left
    assert tok == 1 and info["L"] is None
    tok, info = ts_ref.step(table(i1=1.0), [BEG + 1, 3, BEG + 9], EOT, BEG)  # ... but it may close its pair
    assert tok == BEG + 9


def test_rule4_the_first_id_is_an_early_timestamp():
    z = table(i2=9.0, i6=8.0, i17=7.0, i12=1.0, i13=1.0)
    tok, info = ts_ref.step(z, [], EOT, BEG, max_initial=3)
    assert tok == BEG + 3 and info["M"] is None and "initial" in info["fired"]  # a tie: the larger id
    assert ts_ref.step(z, [], EOT, BEG, max_initial=-1)[0] == BEG + 7
    assert ts_ref.step(z, [], EOT, BEG, max_initial=0)[0] == BEG


def test_rule5_the_summed_probability_of_the_timestamps():
    z = table(i2=1.0)
    z[BEG:] = 0.0  # ten timestamps at 0: L = log 10 = 2.30 > 1, though none of them beats the text logit
    tok, info = ts_ref.step(z, [BEG, 3], EOT, BEG)
    assert tok == BEG + 9 and {"mass", "mass_decided"} <= info["fired"]
    assert info["L"] == pytest.approx(math.log(9.0)) and info["M"] == 1.0  # (tick 0 is masked by rule 3)
    z[2] = 2.5
    tok, info = ts_ref.step(z, [BEG, 3], EOT, BEG)
    assert tok == 2 and "mass" not in info["fired"] and info["gap_lm"] == pytest.approx(2.5 - math.log(9.0))
    z = table(i2=1.0, i12=1.0)  # L = M exactly needs one timestamp alone: not above, text stays allowed
    z[BEG + 3:] = -np.inf
    z[BEG:BEG + 2] = -np.inf
    tok, info = ts_ref.step(z, [], EOT, BEG, max_initial=-1)
    assert tok == BEG + 2 and info["M"] is None
    tok, info = ts_ref.step(z, [BEG, 3], EOT, BEG)
    assert info["L"] == 1.0 and info["M"] == 1.0 and info["gap_lm"] == 0.0 and tok == BEG + 2  # rule 6: the larger id


def test_rule6_ties_and_signed_zeros():
    z = np.full(V, -1.0, np.float32)
    z[1], z[4] = 0.0, -0.0
    tok, info = ts_ref.step(z, [BEG + 9, 2], EOT, BEG)
    assert tok == 4 and info["gap_top"] == 0.0
    z[1], z[4] = -0.0, 0.0
    assert ts_ref.step(z, [BEG + 9, 2], EOT, BEG)[0] == 4
    z = np.full(V, -np.inf, np.float32)  # every logit -inf: the largest allowed id
    assert ts_ref.step(z, [BEG + 9, 2], EOT, BEG)[0] == EOT
    assert ts_ref.step(z, [], EOT, BEG, max_initial=4)[0] == BEG + 4


def test_decode_stops_at_eot_and_at_the_cap():
    def fn(prefix):
        n = len(prefix) - 2
        return table(i2=3.0, i12=2.0) if n < 4 else table(i6=9.0)
    ids, infos = ts_ref.decode(fn, [7, 8], 20, EOT, BEG)
    assert ids == [7, 8, BEG + 2, 2, 2, 2, EOT] and len(infos) == 5
    ids, _ = ts_ref.decode(fn, [7, 8], 4, EOT, BEG)
    assert ids == [7, 8, BEG + 2, 2, 2]  # positions 0 .. 3 fed: 5 ids


PARSER_CASES = [
    ([7, 8, BEG + 1, 2, 3, BEG + 4, BEG + 4, 5, BEG + 6, EOT], [(0, 20, 80, 3, 2, 0), (0, 80, 120, 7, 1, 0)]),
    ([7, 8, BEG + 1, 2, 3, EOT], [(0, 20, 30000, 3, 2, 1)]),               # unclosed at EOT
    ([7, 8, BEG + 1, 2, 3], [(0, 20, 30000, 3, 2, 1)]),                    # unclosed at the cap
    ([7, 8, BEG + 1, 2, BEG + 2, BEG + 5], [(0, 20, 40, 3, 1, 0)]),           # timestamps without text after them
    ([7, 8, BEG + 1, EOT], []),                                             # an opening timestamp alone
    ([7, 8, BEG + 1, 2, BEG + 2, 3, EOT], [(0, 20, 40, 3, 1, 0), (0, 40, 30000, 5, 1, 1)]),  # one timestamp closes and opens
    ([7, 8, 2, 3, BEG + 2, EOT, 4, BEG + 3], [(0, 0, 40, 2, 2, 0)]),       # no opening timestamp; nothing after EOT
    ([7, 8], []),
]


@pytest.mark.parametrize("ids,want", PARSER_CASES)
def test_parser_cases(ids, want):
    assert ts_ref.segments(ids, 2, EOT, BEG) == want


def test_wt_vocab_segments_equals_the_python_parser(pkg, assets):
    _, vocab = assets("micro")
    v = pkg.Vocab(vocab, True)
    info = v.info()
    eot, beg = info["eot"], info["beg"]
    assert (eot, beg) == (tm.EOT, tm.BEG)
    rng = np.random.default_rng(3)
    rows = [[(x - BEG + beg) if x >= BEG else (eot if x == EOT else x) for x in ids] for ids, _ in PARSER_CASES]
    for _ in range(40):  # random rows of text, timestamps (tick 1500 among them) and an occasional EOT
        kinds = rng.choice(3, size=rng.integers(2, 30), p=[0.6, 0.35, 0.05])
        rows.append([50258, 50359] + [int(rng.integers(0, 1000)) if k == 0 else
                                       int(beg + rng.choice([0, 1, 7, 750, 1499, 1500])) if k == 1 else eot for k in kinds])
    for row in rows:
        got = v.segments(row, 2)
        want = ts_ref.segments(row, 2, eot, beg)
        assert [tuple(int(x) for x in g) for g in got] == want, row
    assert v.segments([], 0).size == 0
    with pytest.raises(pkg.WtError):
        v.segments([1, 2], -1)
    v.close()


# ------------------------------------------------------------ the fixture ---

@pytest.fixture(scope="module")
def rows(orc, assets, tmp_path_factory):
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("ts") / "micro-ts.wtw")
    tm.write_model(prefix + ".wtw", p)
    model = orc.Model(p)
    assert model.dims["n_text_ctx"] == tm.N_TEXT_CTX and model.dims["n_vocab"] == tm.N_VOCAB
    out = tm.reference_rows(model, tm.mels(), tm.P_LONG)
    model.close()
    return out


def test_fixture_exercises_every_rule(rows):
    n0 = len(tm.PROMPT)
    closed = []
    for ids, infos in rows:
        first = ids[n0] - tm.BEG
        assert 0 <= first <= 50, first  # the first generated id is a timestamp within max_initial_timestamp
        stamps = [i for i in ids[n0:] if i >= tm.BEG]
        assert stamps == sorted(stamps)  # timestamps never decrease
        assert not any(tm.EOT < i < tm.BEG for i in ids[n0:])
        closed.append(sum(1 for s in ts_ref.segments(ids, n0, tm.EOT, tm.BEG) if not s[5]))
    print("closed segments per clip:", closed, "ids per clip:", [len(ids) for ids, _ in rows])
    assert sum(1 for c in closed if c >= 2) * 2 >= len(rows), closed
    fired = [set().union(*[i["fired"] for i in infos]) for _, infos in rows]
    count = {k: sum(1 for f in fired if k in f) for k in ("mass", "mass_decided", "monotonic_decided", "text_forbidden",
                                                           "text_after_pair")}
    print("clips in which each rule decided:", count)
    assert count["mass_decided"] >= 1   # rule 5 with no single timestamp logit above M
    assert count["monotonic_decided"] >= 1  # rule 3 masked what would otherwise have won
    assert count["text_forbidden"] >= 1 and count["text_after_pair"] >= 1
    # ends before the first segment graph's 32 positions, later, and at the cap
    lens = [len(ids) for ids, _ in rows]
    assert min(lens) < 32 and max(lens) == tm.P_LONG + 1 and any(40 < n < tm.P_LONG for n in lens), lens


def test_fixture_is_decisive(rows):
    gaps = [(min(i["gap_lm"] for i in infos), min(i["gap_top"] for i in infos)) for _, infos in rows]
    print("smallest |L - M| and top-two gap per clip:", [("%.2e" % a, "%.2e" % b) for a, b in gaps])
    indecisive = [b for b, (_, infos) in enumerate(rows) if ts_ref.first_indecisive(infos, tm.MARGIN) is not None]
    assert len(indecisive) * 4 <= len(rows), indecisive


def test_cut_rows_is_the_shorter_decode(orc, assets, tmp_path_factory, rows):
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("ts") / "micro-ts.wtw")
    tm.write_model(prefix + ".wtw", p)
    model = orc.Model(p)
    short = tm.reference_rows(model, tm.mels()[:3], tm.P_SHORT)
    model.close()
    assert [ids for ids, _ in short] == [ids for ids, _ in tm.cut_rows(rows[:3], tm.P_SHORT)]
    assert max(len(ids) for ids, _ in short) == tm.P_SHORT + 1
