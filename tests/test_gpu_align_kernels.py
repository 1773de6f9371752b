"""GPU (-m gpu): the kernels of csrc/k_align.hip (word-level timestamps) one by one through their
debug taps: align_scores against float64 (shapes, head lists, ragged frame counts, guard cells, bit-identity across
batches and cuts, refusals), align_column_stats + align_filter_mean against the float64 restatement of
tests/align_ref.py, and align_dtw bit for bit against align_ref.dtw on the cases the host function wt_dtw_path is held
to.  Without the feature the taps do not exist and every test here fails."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_ref  # noqa: E402

pytestmark = pytest.mark.gpu

# Cost matrix and statistics against float64.  The kernels take the column sums in float64, round mean and 1 / std to
# fp32 once and form Z = (w - mean) * rstd in fp32: three roundings of 2^-24 on a value of size |Z| plus the mean's
# rounding seen through 1 / std; the median picks one of these values and the head mean adds up to 12 of them.
# Measured over the cases below: 9.5e-8 for C, 5.9e-8 relative for the statistics (one fp32
# rounding is 6.0e-8); the bars are a decade above.
C_BOUND = 1e-6       # |C - C64| / max(1, max |C64|)
STATS_BOUND = 6e-7   # relative, mean and 1 / std


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def _weights(rng, clips, heads, L_max, ld, F):
    """Rows that look like attention weights: positive, a few peaks, summing to one over the clip's own frames and zero
    behind them."""
    W = np.zeros((clips, heads, L_max, ld), np.float32)
    for b in range(clips):
        x = rng.standard_normal((heads, L_max, F[b])) * 3.0
        x = np.exp(x - x.max(axis=-1, keepdims=True))
        W[b, :, :, :F[b]] = x / x.sum(axis=-1, keepdims=True)
    return W


def _check_matrix(eng, W, L, F, n_a):
    clips, heads, L_max, ld = W.shape
    N_max = int(max(L)) - n_a - 1
    guard = np.float32(-77.0)
    C0 = np.full((clips, N_max, ld), guard, np.float32)
    S0 = np.full((clips, heads, 2, ld), guard, np.float32)
    C, stats = eng.dbg_align_matrix(W, L, F, n_a, N_max, C0, S0)
    worst_c = worst_s = 0.0
    for b in range(clips):
        Nb, Fb = L[b] - n_a - 1, F[b]
        want = align_ref.cost_matrix(W[b], L[b], Fb, n_a)
        mean, rstd = align_ref.column_stats(W[b], L[b], Fb)
        assert want.shape == (Nb, Fb)
        # cells that belong to no row or frame of the clip are the caller's
        assert np.all(C[b, Nb:] == guard) and np.all(C[b, :, Fb:] == guard) and np.all(stats[b, :, :, Fb:] == guard)
        got = C[b, :Nb, :Fb].astype(np.float64)
        assert np.all(np.isfinite(got))
        worst_c = max(worst_c, float(np.abs(got - want).max() / max(1.0, np.abs(want).max())))
        assert np.array_equal(stats[b, :, 1, :Fb] == 0, rstd == 0)  # a column of equal values, and no other, has rstd = 0
        for k, ref in ((0, mean), (1, rstd)):
            nz = ref != 0
            worst_s = max(worst_s, float((np.abs(stats[b, :, k, :Fb].astype(np.float64) - ref)[nz] / np.abs(ref[nz])).max(initial=0)))
    print(f"align_matrix clips={clips} heads={heads} L={list(L)} F={list(F)}: C err {worst_c:.3g}, stats rel err {worst_s:.3g}")
    assert worst_c <= C_BOUND and worst_s <= STATS_BOUND
    return C, stats


@pytest.mark.parametrize("heads", [1, 2, 12])
def test_cost_matrix_against_float64(eng, heads):
    """L_b in {3, 9, 126} x F_b in {1, 3, 4, 7, 100}: the filter skipped (F <= 3), a window wider than the row (F = 4),
    reflect at both edges; every pair alone and, for 2 heads, all fifteen mixed in one launch."""
    rng = np.random.default_rng(100 + heads)
    pairs = [(L, F) for L in (3, 9, 126) for F in (1, 3, 4, 7, 100)]
    if heads == 2:
        L, F = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
        _check_matrix(eng, _weights(rng, len(pairs), heads, 126, 100, F), L, F, 1)
    else:
        for L, F in pairs:
            Lb, Fb = np.array([L], np.int32), np.array([F], np.int32)
            _check_matrix(eng, _weights(rng, 1, heads, L, F, Fb), Lb, Fb, 1)


def test_cost_matrix_prompt_rows_and_padding(eng):
    """n_a = 4 prompt rows in front (the statistics run over them, the cost does not hold them), rows and frames of W
    behind a clip's own that hold other values, and clips of different sizes next to each other."""
    rng = np.random.default_rng(7)
    L, F = np.array([12, 40, 6], np.int32), np.array([37, 100, 5], np.int32)
    W = _weights(rng, 3, 6, 48, 104, F)
    for b in range(3):
        W[b, :, L[b]:, :] = 0.5   # rows the clip never fed
        W[b, :, :, F[b]:] = 0.25  # frames behind its audio
    _check_matrix(eng, W, L, F, 4)


def test_cost_matrix_column_of_equal_values(eng):
    """std = 0: Z = 0 in that column for that head (Whisper would give NaN), whatever value the column holds; 0.1 does
    not survive a sum of three and a division unchanged."""
    rng = np.random.default_rng(8)
    L, F = np.array([3, 9], np.int32), np.array([7, 100], np.int32)
    W = _weights(rng, 2, 2, 9, 100, F)
    W[0, 0, :, 2] = 0.1
    W[0, 1, :, 6] = 0.0
    W[1, 1, :, 50] = np.float32(1.0 / 3.0)
    W[1, :, :, 99] = 0.7
    C, stats = _check_matrix(eng, W, L, F, 0)
    assert stats[0, 0, 1, 2] == 0 and stats[0, 1, 1, 6] == 0 and stats[1, 1, 1, 50] == 0 and np.all(stats[1, :, 1, 99] == 0)


def test_cost_matrix_refusals(eng, pkg):
    W = np.zeros((1, 2, 8, 16), np.float32)
    one = lambda v: np.array([v], np.int32)  # noqa: E731
    for L, F, n_a, N_max in ((9, 16, 1, 7), (2, 16, 1, 1), (8, 0, 1, 6), (8, 17, 1, 6), (8, 16, 1, 5), (8, 16, -1, 8)):
        with pytest.raises(pkg.WtError) as err:
            eng.dbg_align_matrix(W, one(L), one(F), n_a, N_max)
        assert err.value.code == 1
    with pytest.raises(pkg.WtError) as err:  # the launcher's own: more than 128 heads, more than 1500 frames
        eng.dbg_align_matrix(np.zeros((1, 129, 3, 4), np.float32), one(3), one(4), 0, 2)
    assert err.value.code == 1
    with pytest.raises(pkg.WtError) as err:
        eng.dbg_align_matrix(np.zeros((1, 1, 3, 1501), np.float32), one(3), one(4), 0, 2)
    assert err.value.code == 1
    C, _ = eng.dbg_align_matrix(W + 0.5, one(8), one(16), 1, 6)  # the engine is usable afterwards
    assert np.all(C == 0)


# ------------------------------------------------------------------ DTW ---
def _run_dtw(eng, mats, N_max=None, ld=None):
    """One launch over the matrices `mats` (clip b: its own N_b x F_b in the corner of [N_max][ld], other values
    around it); jump and the trace codes must equal align_ref.dtw's, cells of no clip must come back untouched."""
    clips = len(mats)
    N_max = N_max or max(m.shape[0] for m in mats)
    ld = ld or max(m.shape[1] for m in mats)
    C = np.full((clips, N_max, ld), -1000.0, np.float32)  # an attractive cost outside: reading it would show
    N, F = np.zeros(clips, np.int32), np.zeros(clips, np.int32)
    for b, m in enumerate(mats):
        N[b], F[b] = m.shape
        C[b, :N[b], :F[b]] = m
    jump0 = np.full((clips, N_max), -9, np.int32)
    trace0 = np.full((clips, N_max, ld), 99, np.uint8)
    jump, trace = eng.dbg_align_dtw(C, N, F, jump0, trace0)
    for b, m in enumerate(mats):
        want_jump, _, want_trace, _ = align_ref.dtw(m)
        assert np.array_equal(jump[b, :N[b]], want_jump), (b, m.shape)
        assert np.all(jump[b, N[b]:] == 0)
        assert np.array_equal(trace[b, :N[b], :F[b]], want_trace), (b, m.shape)
        assert np.all(trace[b, N[b]:] == 99) and np.all(trace[b, :, F[b]:] == 99)
    return jump


def test_dtw_named_and_seeded_cases(eng):
    cases = dict(align_ref.dtw_cases())
    small = [C for name, C in cases.items() if max(C.shape) <= 24]
    assert len(small) >= 500
    _run_dtw(eng, small)                           # one wavefront per clip
    for name in ("n1", "f1", "one_cell", "n2_f3", "all_equal", "all_zero", "signed_zero"):
        _run_dtw(eng, [cases[name]])               # each alone, at its own size
    _run_dtw(eng, [cases["n_above_f"]])            # 40 x 7
    jump = _run_dtw(eng, [cases["staircase"]])
    assert list(jump[0]) == [3 * r for r in range(12)]


def test_dtw_largest_clip(eng):
    _run_dtw(eng, [dict(align_ref.dtw_cases())["full"]])  # 447 x 1500: eight wavefronts, 1946 diagonals


def test_dtw_32_clips_of_different_sizes(eng):
    """Four and eight wavefronts per block, with clips of one wavefront's size among them, and a clip without rows."""
    rng = np.random.default_rng(31)
    for top in (200, 300):
        mats = [rng.standard_normal((int(rng.integers(1, top + 1)), int(rng.integers(1, 260)))).astype(np.float32) for _ in range(30)]
        mats += [rng.integers(0, 2, (top, 259)).astype(np.float32), rng.standard_normal((65, 1)).astype(np.float32)]
        _run_dtw(eng, mats)
    C = np.zeros((2, 5, 6), np.float32)
    jump, trace = eng.dbg_align_dtw(C, np.array([0, 5], np.int32), np.array([6, 6], np.int32), np.full((2, 5), -9, np.int32))
    assert np.all(jump[0] == 0) and np.all(trace[0] == 0) and list(jump[1]) == [0, 0, 0, 0, 0]


def test_dtw_refusals(eng, pkg):
    one = lambda v: np.array([v], np.int32)  # noqa: E731
    C = np.zeros((1, 4, 6), np.float32)
    for N, F in ((5, 6), (-1, 6), (4, 7), (4, 0)):
        with pytest.raises(pkg.WtError) as err:
            eng.dbg_align_dtw(C, one(N), one(F))
        assert err.value.code == 1
    for shape in ((1, 448, 4), (1, 4, 1501)):
        with pytest.raises(pkg.WtError) as err:
            eng.dbg_align_dtw(np.zeros(shape, np.float32), one(4), one(4))
        assert err.value.code == 1
    jump, _ = eng.dbg_align_dtw(C, one(4), one(6))
    assert list(jump[0]) == [0, 0, 0, 0]


# ---------------------------------------------------------------- scores ---
def _softmax2(S, F):
    """S [..., T] log2-domain scores in float64 -> weights over t < F, zero behind."""
    W = np.zeros_like(S)
    x = S[..., :F]
    x = np.exp2(x - x.max(axis=-1, keepdims=True))
    W[..., :F] = x / x.sum(axis=-1, keepdims=True)
    return W


def _scores_case(rng, B, H, T, n_pos, spread=13.0):
    """Queries and encoder output whose scores have a standard deviation of `spread` log2 units (+-40 at three sigma)."""
    d = 64 * H
    E = rng.standard_normal((B, T, d)).astype(np.float32)
    qp = (rng.standard_normal((n_pos, B, H * d)) * (spread / np.sqrt(d))).astype(np.float32)
    return qp, E


def _check_scores(eng, qp, E, head, slot, heads_total, F, pos0, mode=1):
    n_pos, B, _ = qp.shape
    T, d = E.shape[1], E.shape[2]
    L_max, ld = pos0 + n_pos + 2, T + 4  # two guard rows behind the pass, four guard frames behind T
    guard = np.float32(-55.0)
    W0 = np.full((B, heads_total, L_max, ld), guard, np.float32)
    W = eng.dbg_align_scores(qp, E, head, slot, F, W0, pos0, mode)
    written = np.zeros(W.shape, bool)
    worst, lo, hi = 0.0, np.inf, -np.inf
    E64, q64 = E.astype(np.float64), qp.astype(np.float64)
    for b in range(B):
        for h, s in zip(head, slot):
            S = np.einsum("pd,td->pt", q64[:, b, h * d:(h + 1) * d], E64[b])
            lo, hi = min(lo, S[:, :F[b]].min()), max(hi, S[:, :F[b]].max())
            want = _softmax2(S, F[b])
            got = W[b, s, pos0:pos0 + n_pos, :T].astype(np.float64)
            written[b, s, pos0:pos0 + n_pos, :T] = True
            assert np.all(got[:, F[b]:] == 0), "frames behind the clip's audio are zero"
            big = want > 1e-30
            worst = max(worst, float((np.abs(got - want)[big] / want[big]).max()))
            assert np.all(got[~big] < 1e-29)
            assert np.abs(got.sum(axis=-1) - 1).max() < 1e-5
    assert np.all(W[~written] == guard), "rows of other positions, slots of other heads and the guard frames are the caller's"
    print(f"align_scores mode={mode} B={B} d={d} T={T} pos0={pos0} np={n_pos} heads={list(head)} F={sorted(set(F.tolist()))}: "
          f"scores {lo:.1f} .. {hi:.1f}, W rel err {worst:.3g}")
    assert worst <= W_BOUND
    return W


# |W - W64| / W64 over the weights above 1e-30.  A score is a d_model-long fp32-level contraction (two fp16 planes, three
# products, fp32 accumulation: DESIGN.md section 4.1 measures ~1e-6 of |q||e|), here |q||e| ~ 13 sqrt(d) <= 260, and a
# weight's relative error is ln 2 times its score's absolute error plus the exp2 and the normalisation, a few 2^-24.
# Measured over the cases below, both forms of the kernel: 3.0e-5 (d_model 384, T = 1500, scores
# -57 .. 69), 2.5e-5 at T = 100.  A decade above that is 3e-4; the bar is the lower 1e-4, above which an error is a bug of the contraction.
W_BOUND = 1e-4


@pytest.mark.parametrize("H,B,pos0,n_pos", [(2, 1, 0, 1), (2, 3, 2, 5), (6, 3, 2, 5), (2, 32, 0, 4), (6, 32, 0, 4), (2, 1, 96, 32),
                                             (6, 1, 96, 32), (6, 64, 5, 2)])
@pytest.mark.parametrize("mode", [0, 1])
def test_scores_against_float64(eng, H, B, pos0, n_pos, mode):
    """T = 100 (six 16-frame tiles and 4 frames), F_b from {1, 3, 37, T} mixed inside the batch, every head of the layer."""
    rng = np.random.default_rng(1000 * H + 10 * B + n_pos)
    T = 100
    qp, E = _scores_case(rng, B, H, T, n_pos)
    F = np.array([(1, 3, 37, T)[(b + B) % 4] for b in range(B)], np.int32)
    if B >= 4:
        assert set(F.tolist()) == {1, 3, 37, T}
    _check_scores(eng, qp, E, np.arange(H), np.arange(H), H, F, pos0, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_scores_head_lists(eng, mode):
    """One head, and {0, 5} of 6 written to slots 3 and 1 of 4: the other heads are not computed, the other slots not
    written."""
    rng = np.random.default_rng(12)
    qp, E = _scores_case(rng, 3, 6, 100, 5)
    F = np.array([37, 100, 3], np.int32)
    _check_scores(eng, qp, E, np.array([4]), np.array([0]), 1, F, 2, mode)
    _check_scores(eng, qp, E, np.array([0, 5]), np.array([3, 1]), 4, F, 2, mode)
    qp, E = _scores_case(rng, 2, 2, 100, 3)
    _check_scores(eng, qp, E, np.array([1]), np.array([1]), 2, np.array([100, 1], np.int32), 0, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_scores_full_length_clip(eng, mode):
    """T = 1500 once per form: 94 tiles, the last of 12 frames (twelve chunks of eight tiles, the last of six); d_model
    384, 32 positions, F = T and a short clip."""
    rng = np.random.default_rng(13)
    qp, E = _scores_case(rng, 2, 6, 1500, 32)
    _check_scores(eng, qp, E, np.array([1, 4]), np.array([0, 1]), 2, np.array([1500, 205], np.int32), 0, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_scores_bits_do_not_depend_on_the_batch_or_the_cut(eng, mode):
    rng = np.random.default_rng(14)
    B, H, T, n_pos, pos0 = 3, 6, 100, 5, 2
    qp, E = _scores_case(rng, B, H, T, n_pos)
    F = np.array([37, 100, 3], np.int32)
    head = slot = np.arange(H)
    whole = _check_scores(eng, qp, E, head, slot, H, F, pos0, mode)
    for b in range(B):  # the clip alone
        alone = _check_scores(eng, qp[:, b:b + 1], E[b:b + 1], head, slot, H, F[b:b + 1], pos0, mode)
        assert np.array_equal(alone[0].view(np.uint32), whole[b].view(np.uint32))
    W0 = np.full(whole.shape, np.float32(-55.0), np.float32)  # the same positions in two launches
    two = eng.dbg_align_scores(qp[:2], E, head, slot, F, W0, pos0, mode)
    two = eng.dbg_align_scores(qp[2:], E, head, slot, F, two, pos0 + 2, mode)
    assert np.array_equal(two.view(np.uint32), whole.view(np.uint32))


def test_scores_refusals(eng, pkg):
    rng = np.random.default_rng(15)
    qp, E = _scores_case(rng, 2, 2, 100, 3)
    F = np.array([100, 50], np.int32)
    W = np.zeros((2, 2, 8, 104), np.float32)
    ok = dict(qp=qp, E=E, head=np.array([0, 1]), slot=np.array([0, 1]), F=F, W=W, pos0=0)
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
           dict(qp=_scores_case(rng, 2, 2, 100, 65)[0], W=np.zeros((2, 2, 70, 104), np.float32)),  # 130 rows in a pass
           dict(E=np.zeros((2, 98, 128), np.float32)),                 # T % 4 != 0
           dict(qp=np.zeros((3, 2, 3 * 192), np.float32), E=np.zeros((2, 100, 192), np.float32),
                W=np.zeros((2, 2, 8, 104), np.float32))]               # a d_model without a kernel
    for change in bad:
        with pytest.raises(pkg.WtError) as err:
            eng.dbg_align_scores(**{**ok, **change})
        assert err.value.code == 1, change.keys()
    _check_scores(eng, qp, E, np.array([0, 1]), np.array([0, 1]), 2, F, 0)  # the engine is usable afterwards
