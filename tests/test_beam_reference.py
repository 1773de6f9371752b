"""The reference beam search of tests/beam_ref.py (the yardstick of tests/test_gpu_beam.py) against the rules of
DESIGN.md section 11: greedy at K = 1 on the CPU oracle, and hand-made logits tables for EOT finishing, the
max-length fill and both tie rules.  CPU only."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_ref  # noqa: E402

EOT = 0  # the tables' EOT: the smallest id, so that equal logits rank it last


def table(rows):
    """logits_fn from {prefix length: logits} (every hypothesis of a length sees the same row)."""
    return lambda prefix: np.asarray(rows[len(prefix)], np.float32)


def lp(z):
    return beam_ref.log_softmax64(np.asarray(z, np.float32))


def test_k1_is_greedy_on_micro(orc, assets):
    prefix, _ = assets("micro")
    model = orc.Model(prefix + ".wtw")
    rng = np.random.default_rng(1234)
    prompt = [3, 5, 7, 11]
    for b in range(2):
        mel = rng.uniform(-1.0, 1.5, size=(80, 200)).astype(np.float32)
        enc = model.encode(mel)
        ids, _ = model.decode_greedy(enc, prompt, 14, 50257, True)
        fn = beam_ref.oracle_logits_fn(model, enc, 50257)
        r = beam_ref.beam_search(fn, prompt, 1, 14, 50257)
        assert r["ids"] == [int(i) for i in ids]
        assert r["n_gen"] == len(ids) - len(prompt)
        assert abs(r["sum"] - beam_ref.teacher_forced_sum(fn, r["ids"], len(prompt))) < 1e-9
    model.close()


def test_equal_logits_larger_id_first_then_lower_slot_first():
    z = [0.0] * 6
    fn = table({1: z, 2: z, 3: z})
    # one step: the top ranks of a uniform row are ids 5, 4, 3; the live slots get 5 and 4
    r = beam_ref.beam_search(fn, [1], 2, 1, EOT)
    assert r["ids"] == [1, 5] and r["n_gen"] == 1 and not r["done_early"]
    assert r["margin"] == 0.0  # every decision was a tie
    # two steps: all six candidates have one score; slot 0's ranks 0 and 1 come before slot 1's rank 0
    r = beam_ref.beam_search(fn, [1], 2, 2, EOT)
    assert r["ids"] == [1, 5, 5]
    assert math.isclose(r["sum"], 2 * math.log(1 / 6))


def test_eot_finishes_hypotheses_and_the_clip():
    z1 = [3.0, 2.0, 1.0, 0.0, 0.0, 0.0]  # EOT first, then ids 1 and 2
    z2 = [5.0, 0.0, 0.0, 0.0, 0.0, 0.0]  # every hypothesis of length 2 ends
    fn = table({1: z1, 2: z2, 3: z2})
    r = beam_ref.beam_search(fn, [1], 2, 3, EOT)
    # step 0: [EOT] finished (sum lp1[0]), live [1] and [2]; step 1: [1, EOT] fills the list, the clip is done
    assert r["done_early"] and r["eot_slots"] == [0, 0]
    a, b = lp(z1)[0], lp(z1)[1] + lp(z2)[0]
    best = [1, EOT] if a / 1 >= b / 2 else [1, 1, EOT]
    assert r["ids"] == best
    assert math.isclose(r["sum"], a if a / 1 >= b / 2 else b)


def test_max_length_fills_the_list_from_the_live_slots():
    z = [-5.0, 0.0, 0.0, 0.0, 0.0, 2.0]  # EOT never reaches the walk's cut
    fn = table({1: z, 2: z, 3: z, 4: z})
    r = beam_ref.beam_search(fn, [1], 3, 3, EOT)
    assert not r["done_early"] and r["eot_slots"] == []
    assert r["n_gen"] == 3 and r["ids"] == [1, 5, 5, 5]
    assert math.isclose(r["sum"], 3 * lp(z)[5])


def test_eot_from_a_later_slot_and_the_length_normalisation():
    # step 0: live [5] (slot 0) and [4] (slot 1); step 1: slot 1's row puts EOT first, slot 0's does not
    z1 = [-9.0, 0.0, 0.0, 0.0, 1.0, 1.5]
    z_after5 = [-9.0, 0.0, 0.0, 0.0, 0.0, 3.0]
    z_after4 = [4.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    fn = lambda p: np.asarray(z1 if len(p) == 1 else (z_after5 if p[-1] == 5 else z_after4), np.float32)  # noqa: E731
    r = beam_ref.beam_search(fn, [1], 2, 2, EOT)
    assert r["eot_slots"] == [1]
    fin_eot = lp(z1)[4] + lp(z_after4)[0]
    live0 = lp(z1)[5] + lp(z_after5)[5]
    # the list: [4, EOT] (from the walk), then the best live hypothesis [5, 5]; both have two generated ids
    expect = [1, 4, EOT] if fin_eot >= live0 else [1, 5, 5]
    assert r["ids"] == expect and r["n_gen"] == 2
