"""GPU (-m gpu): the bf16 form of align_scores (k_align.hip, option full_bf16_all) through the tap
wt_dbg_align_scores_bf16, and the conversion kernel f32_to_bf16 through wt_dbg_f32_to_bf16.  W against float64 on the
bf16-rounded q' and E at the bar of tests/test_gpu_align_kernels.py (tests/test_full_bf16_all_reference.py shows on the
CPU that the reference's own arithmetic stays under a quarter of it), rows summing to one, exact zeros behind a clip's
frames, guard cells, the bits of a column independent of the batch, its neighbours and the cut of the positions into
launches, head and slot lists, the launcher's refusals.  Without the feature the taps do not exist and every test here
fails."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_bf16_ref as ab  # noqa: E402
from decoder_attn_ref import bf16_round  # noqa: E402

pytestmark = pytest.mark.gpu

observed = {"rel": 0.0}


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()
    print(f"align_scores bf16: largest W relative error against float64 on the rounded operands {observed['rel']:.3g} "
          f"(bar {ab.W_BOUND:.3g})")


def _check_scores(eng, qp, E, head, slot, heads_total, F, pos0, mode=1):
    n_pos, B, _ = qp.shape
    T, d = E.shape[1], E.shape[2]
    L_max, ld = pos0 + n_pos + 2, T + 4  # two guard rows behind the pass, four guard frames behind T
    guard = np.float32(-55.0)
    W0 = np.full((B, heads_total, L_max, ld), guard, np.float32)
    W = eng.dbg_align_scores(qp, E, head, slot, F, W0, pos0, mode, bf16=True)
    written = np.zeros(W.shape, bool)
    worst, lo, hi = 0.0, np.inf, -np.inf
    for b in range(B):
        for h, s in zip(head, slot):
            S = ab.scores64(qp, E, b, int(h))
            lo, hi = min(lo, S[:, :F[b]].min()), max(hi, S[:, :F[b]].max())
            want = ab.softmax2(S, F[b])
            got = W[b, s, pos0:pos0 + n_pos, :T].astype(np.float64)
            written[b, s, pos0:pos0 + n_pos, :T] = True
            assert np.all(got >= 0) and np.all(got[:, F[b]:] == 0), "frames behind the clip's audio are zero"
            rel, small = ab.relative_error(got, want)
            worst = max(worst, rel)
            assert small < 1e-29
            assert np.abs(got.sum(axis=-1) - 1).max() < 1e-5
    assert np.all(W[~written] == guard), "rows of other positions, slots of other heads and the guard frames are the caller's"
    observed["rel"] = max(observed["rel"], worst)
    print(f"align_scores bf16 mode={mode} B={B} d={d} T={T} pos0={pos0} np={n_pos} heads={list(head)} F={sorted(set(F.tolist()))}: "
          f"scores {lo:.1f} .. {hi:.1f}, W rel err {worst:.3g}")
    assert worst <= ab.W_BOUND
    return W


@pytest.mark.parametrize("H,B,pos0,n_pos", ab.SHAPES)
@pytest.mark.parametrize("mode", [0, 1])
def test_scores_against_float64(eng, H, B, pos0, n_pos, mode):
    """T = 100 (six 16-frame tiles and 4 frames), F_b from {1, 3, 37, T} mixed inside the batch, every head of the layer."""
    T = ab.T_SHORT
    qp, E = ab.case(H, B, T, n_pos, ab.seed_of(H, B, n_pos, T))
    F = ab.frames(B, T)
    if B >= 4:
        assert set(F.tolist()) == {1, 3, 37, T}
    _check_scores(eng, qp, E, np.arange(H), np.arange(H), H, F, pos0, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_scores_full_length_clip(eng, mode):
    """T = 1500 once per form: 94 tiles, the last of 12 frames; d_model 384, 32 positions, F = T and a short clip."""
    H, B, pos0, n_pos = ab.LONG_SHAPE
    qp, E = ab.case(H, B, ab.T_LONG, n_pos, ab.seed_of(H, B, n_pos, ab.T_LONG))
    _check_scores(eng, qp, E, np.array([1, 4]), np.array([0, 1]), 2, np.array([1500, 205], np.int32), pos0, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_scores_head_lists(eng, mode):
    """One head, and {0, 5} of 6 written to slots 3 and 1 of 4: the other heads are not computed, the other slots not
    written."""
    qp, E = ab.case(6, 3, 100, 5, 12)
    F = np.array([37, 100, 3], np.int32)
    _check_scores(eng, qp, E, np.array([4]), np.array([0]), 1, F, 2, mode)
    _check_scores(eng, qp, E, np.array([0, 5]), np.array([3, 1]), 4, F, 2, mode)
    qp, E = ab.case(2, 2, 100, 3, 13)
    _check_scores(eng, qp, E, np.array([1]), np.array([1]), 2, np.array([100, 1], np.int32), 0, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_scores_bits_do_not_depend_on_the_batch_or_the_cut(eng, mode):
    B, H, T, n_pos, pos0 = 3, 6, 100, 5, 2
    qp, E = ab.case(H, B, T, n_pos, 14)
    F = np.array([37, 100, 3], np.int32)
    head = slot = np.arange(H)
    whole = _check_scores(eng, qp, E, head, slot, H, F, pos0, mode)
    for b in range(B):  # the clip alone
        alone = _check_scores(eng, qp[:, b:b + 1], E[b:b + 1], head, slot, H, F[b:b + 1], pos0, mode)
        assert np.array_equal(alone[0].view(np.uint32), whole[b].view(np.uint32))
    for h in (0, 3):  # a head alone: its columns do not depend on their neighbours
        one = _check_scores(eng, qp, E, np.array([h]), np.array([0]), 1, F, pos0, mode)
        assert np.array_equal(one[:, 0].view(np.uint32), whole[:, h].view(np.uint32))
    W0 = np.full(whole.shape, np.float32(-55.0), np.float32)  # the same positions in two launches
    two = eng.dbg_align_scores(qp[:2], E, head, slot, F, W0, pos0, mode, bf16=True)
    two = eng.dbg_align_scores(qp[2:], E, head, slot, F, two, pos0 + 2, mode, bf16=True)
    assert np.array_equal(two.view(np.uint32), whole.view(np.uint32))


def test_the_query_is_rounded_in_the_kernel(eng):
    """q' given in fp32 and q' given already rounded to bf16 are the same launch, bit for bit; the fp32 form is another."""
    qp, E = ab.case(2, 3, 100, 5, 16)
    F = np.array([37, 100, 3], np.int32)
    W0 = np.zeros((3, 2, 8, 104), np.float32)
    a = eng.dbg_align_scores(qp, E, np.arange(2), np.arange(2), F, W0, 0, 1, bf16=True)
    b = eng.dbg_align_scores(bf16_round(qp).reshape(qp.shape), E, np.arange(2), np.arange(2), F, W0, 0, 1, bf16=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c = eng.dbg_align_scores(qp, E, np.arange(2), np.arange(2), F, W0, 0, 1)
    assert not np.array_equal(a.view(np.uint32), c.view(np.uint32))


def test_scores_refusals(eng, pkg):
    qp, E = ab.case(2, 2, 100, 3, 15)
    F = np.array([100, 50], np.int32)
    W = np.zeros((2, 2, 8, 104), np.float32)
    ok = dict(qp=qp, E=E, head=np.array([0, 1]), slot=np.array([0, 1]), F=F, W=W, pos0=0, bf16=True)
    bad = [dict(head=np.array([2]), slot=np.array([0])),               # a head >= H
           dict(head=np.zeros(0, np.int32), slot=np.zeros(0, np.int32)),  # no heads
           dict(head=np.array([0]), slot=np.array([2])),               # a slot W does not have
           dict(head=np.array([0, 1]), slot=np.array([1, 1])),         # two heads into one slot
           dict(head=np.array([1, 1]), slot=np.array([0, 1])),         # a head listed twice
           dict(mode=2), dict(mode=-1),
           dict(F=np.array([0, 50], np.int32)), dict(F=np.array([100, 101], np.int32)),
           dict(pos0=6), dict(pos0=-1),                                # rows W does not have
           dict(W=np.zeros((2, 2, 8, 102), np.float32)),               # a row stride that is no multiple of 4
           dict(W=np.zeros((2, 2, 8, 96), np.float32)),                # ... or shorter than T
           dict(qp=ab.case(2, 2, 100, 65, 15)[0], W=np.zeros((2, 2, 70, 104), np.float32)),  # 130 rows in a pass
           dict(E=np.zeros((2, 98, 128), np.float32)),                 # T % 4 != 0
           dict(qp=np.zeros((3, 2, 3 * 192), np.float32), E=np.zeros((2, 100, 192), np.float32),
                W=np.zeros((2, 2, 8, 104), np.float32))]               # a d_model without a kernel
    for change in bad:
        with pytest.raises(pkg.WtError) as err:
            eng.dbg_align_scores(**{**ok, **change})
        assert err.value.code == 1, change.keys()
    _check_scores(eng, qp, E, np.array([0, 1]), np.array([0, 1]), 2, F, 0)  # the engine is usable afterwards


@pytest.mark.parametrize("n", [4, 128 * 100, 3 * 1500 * 384])
def test_f32_to_bf16_is_the_rounding_to_nearest_even(eng, pkg, n):
    """Exact against decoder_attn_ref.bf16_round: random values, ties (both ways), denormals, infinities, the largest
    finite value (rounds to infinity); the guard cells behind the plane come back as given."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
    special = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0x3F807FFF, 0x3F808001, 0x00000001, 0x00008000, 0x7F800000,
                        0xFF800000, 0x7F7FFFFF, 0x80000000, 0x00000000], np.uint32).view(np.float32)
    x[: min(n, special.size)] = special[: min(n, special.size)]
    guard = 8
    out0 = np.full(n + guard, -3.0, np.float32)
    out = eng.dbg_f32_to_bf16(x, out0)
    assert np.array_equal(out[:n].view(np.uint32), bf16_round(x).view(np.uint32))
    assert np.all(out[n:] == -3.0)
    if n == 4:
        for bad in (3, 6):
            with pytest.raises(pkg.WtError) as err:
                eng.dbg_f32_to_bf16(np.zeros(bad, np.float32), np.zeros(bad, np.float32))
            assert err.value.code == 1
