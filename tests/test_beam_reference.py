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


def test_ranked_prefix_is_the_full_order_prefix():
    rng = np.random.default_rng(7)
    for V in (6, 50, 4097):
        lp = rng.integers(-4, 4, V).astype(np.float64)  # many exact ties
        lp[rng.integers(0, V, 3)] = -math.inf
        full = beam_ref.ranked(lp)
        for n in (1, 3, 9, V):
            assert list(beam_ref.ranked(lp, n)) == list(full[:n])


def test_signed_zeros_are_one_logit():
    # ids 3 (-0) and 2 (+0) are equal logits: the larger id first, whichever zero it holds
    z = np.array([-3.0, -1.0, 0.0, -0.0, -2.0, -2.5], np.float32)
    assert list(beam_ref.ranked(lp(z))[:2]) == [3, 2]
    fn = table({1: z, 2: z})
    r = beam_ref.beam_search(fn, [1], 2, 1, EOT)
    assert r["ids"] == [1, 3]
    assert r["gaps"]["logit"][0] == 0.0
    z2 = z.copy()
    z2[[2, 3]] = z[[3, 2]]  # the signs swapped: the same order
    assert list(beam_ref.ranked(lp(z2))) == list(beam_ref.ranked(lp(z)))


def test_minus_inf_entries_and_a_masked_chunk():
    # a row whose first 4096 entries (one whole top-k chunk of the kernels) are -inf: they take no probability and rank
    # last; the decision gaps stay numbers
    V = 8192 + 5
    z = np.full(V, -20.0, np.float32)
    z[:4096] = -np.inf
    z[[5000, 6000, 7000, 8196]] = [1.0, 2.0, 2.0, 0.5]
    want = lp(z[4096:])
    got = lp(z)
    assert np.all(np.isneginf(got[:4096])) and np.array_equal(got[4096:], want)
    fn = table({1: z, 2: z, 3: z})
    r = beam_ref.beam_search(fn, [1], 3, 3, EOT)
    assert r["ids"] == [1, 7000, 7000, 7000]
    assert all(not math.isnan(g) for k in beam_ref.GAP_KINDS for g in r["gaps"][k])
    # few finite entries: the -inf ones fill the ranks after them, larger id first
    z = np.full(12, -np.inf, np.float32)
    z[[4, 9]] = [0.0, 1.0]
    assert list(beam_ref.ranked(lp(z))[:4]) == [9, 4, 11, 10]


def test_gap_kinds_and_dropped_eot():
    # ids 5 and 4 tie at the top, ids 3 and 2 at ranks K+1 / K+2; the two live slots share a sum, so at step 1 slot 0's
    # rank 1 and slot 1's rank 0 tie where the walk ends
    z = [-1.0, -1.0, 0.0, 0.0, 1.0, 1.0]
    r = beam_ref.beam_search(table({1: z, 2: z, 3: z}), [1], 2, 2, EOT)
    assert r["gaps"]["logit"][0] == 0.0 and r["gaps"]["logit"][1] > 0.0
    assert r["gaps"]["cut"][0] == 0.0 and r["gaps"]["score"] == [0.0]
    assert r["ids"] == [1, 5, 5] and r["gaps"]["final"] == [0.0]  # two lists of equal sum and length: the first wins
    # EOT first in every row: step 0 finishes one, step 1 offers it from both slots with one list place left
    z1 = [3.0, 2.0, 2.0, 0.0, 0.0, 0.0]
    z2 = [5.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    r = beam_ref.beam_search(table({1: z1, 2: z2}), [1], 2, 2, EOT)
    assert r["done_early"] and r["eot_slots"] == [0, 0] and r["eot_dropped"] == 1
    # [1, EOT] (sum lp1[0] over 1) against [2, EOT] (lp1[2] + lp2[0] over 2): the final ranking
    assert len(r["gaps"]["final"]) == 1
