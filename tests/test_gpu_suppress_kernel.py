"""suppress_logits (k_suppress.hip) through its debug tap: the cells it writes and the cells it
leaves, at the chunk edges of the kernels behind it, and then the masked rows through the taps of those kernels —
ts_select, the sampler, the scores and a step of full-length beam search — against tests/suppress_ref.py in front of their
own references, at the bars their own tests use.  Without the feature the tap does not exist and every test here fails."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_full_ref as bfr  # noqa: E402
import sample_ref  # noqa: E402
import scores_ref  # noqa: E402
import suppress_ref as sup  # noqa: E402
import ts_ref  # noqa: E402
from test_gpu_beam_full_kernels import LP_BOUND, LSE_BOUND, N0, PROMPT, Chain  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = "WT_ERR_INVALID_ARG"
SHAPES = [(4101, 4104), (8192, 8200), (51865, 51868)]  # (V, ldl): ldl > V, rows 16-byte aligned as the engine's
DEN_BOUND = 8.6e-7  # tests/test_gpu_scores_kernel.py / test_gpu_beam_full_kernels.py: the logsumexp bar of the score kernels


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def rows_of(rows, ldl, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, ldl)) * 3.0).astype(np.float32)


def expect(z, V, ids, first_ids, first):
    want = z.copy()
    for i in list(ids) + (list(first_ids) if first else []):
        if 0 <= i < V:
            want[:, i] = -np.inf
    return want


@pytest.mark.parametrize("V,ldl", SHAPES)
@pytest.mark.parametrize("rows", [1, 128])
def test_only_the_listed_cells_change(eng, V, ldl, rows):
    z = rows_of(rows, ldl, V + rows)
    ids = [0, 4095, 4096, V - 1, 4095, 17]  # the chunk edges of the select kernels, the row's ends, a duplicate
    first_ids = [1, V - 2, 4096]
    for first in (False, True):
        got = eng.dbg_suppress_logits(z, ids, first_ids, first, V=V)
        want = expect(z, V, ids, first_ids, first)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))  # bit for bit, the padding columns included
        assert np.array_equal(got[:, V:], z[:, V:])
        assert np.isneginf(got[:, [0, 4095, 4096, V - 1, 17]]).all()
        assert np.isneginf(got[:, [1, V - 2]]).all() == first


def test_empty_lists_change_nothing(eng):
    z = rows_of(3, 4104, 5)
    assert np.array_equal(eng.dbg_suppress_logits(z, [], [], True, V=4101).view(np.uint32), z.view(np.uint32))
    # a first-list alone, without the flag
    assert np.array_equal(eng.dbg_suppress_logits(z, [], [7, 8], False, V=4101).view(np.uint32), z.view(np.uint32))
    got = eng.dbg_suppress_logits(z, [], [7, 8], True, V=4101)
    assert np.isneginf(got[:, [7, 8]]).all() and np.isfinite(got).sum() == z.size - 6


def test_an_id_outside_the_vocabulary_is_skipped(eng):
    """The list is data to the kernel: nothing beyond column V - 1 is touched, whatever it holds."""
    V, ldl = 4101, 4104
    z = rows_of(2, ldl, 9)
    got = eng.dbg_suppress_logits(z, [V, V + 2, ldl, 1 << 20, -1, 1 << 40, 5], [], False, V=V)
    assert np.array_equal(got.view(np.uint32), expect(z, V, [5], [], False).view(np.uint32))


def test_full_lists(eng):
    V, ldl = 8192, 8200
    z = rows_of(2, ldl, 11)
    rng = np.random.default_rng(3)
    ids, first_ids = rng.integers(0, V, 1024), rng.integers(0, V, 1024)
    for first in (False, True):
        got = eng.dbg_suppress_logits(z, ids, first_ids, first, V=V)
        assert np.array_equal(got.view(np.uint32), expect(z, V, ids, first_ids, first).view(np.uint32))


def test_refusals(pkg, eng):
    def status(**kw):
        a = dict(rows=2, V=4101, ldl=4104, n=1, n_first=1)
        a.update(kw)
        z = np.zeros((max(a["rows"], 1), max(a["ldl"], 1)), np.float32)
        out = np.zeros_like(z)
        ids = np.zeros(2048, np.int64)
        rc = pkg.lib().wt_dbg_suppress_logits(eng.handle, a["rows"], a["V"], a["ldl"], pkg._fp(z), pkg._fp(out), pkg._ip64(ids),
                                              a["n"], pkg._ip64(ids), a["n_first"], 0)
        return pkg.STATUS_NAMES[rc]

    assert status() == "WT_OK"
    assert status(rows=0) == INVALID and status(rows=129) == INVALID
    assert status(ldl=4100) == INVALID and status(V=0) == INVALID
    assert status(n=1025) == INVALID and status(n_first=1025) == INVALID and status(n=-1) == INVALID
    z = np.zeros((1, 8), np.float32)
    L = pkg.lib()
    assert pkg.STATUS_NAMES[L.wt_dbg_suppress_logits(eng.handle, 1, 8, 8, None, pkg._fp(z), None, 0, None, 0, 0)] == INVALID
    assert pkg.STATUS_NAMES[L.wt_dbg_suppress_logits(eng.handle, 1, 8, 8, pkg._fp(z), pkg._fp(z), None, 1, None, 0, 0)] == INVALID
    assert pkg.STATUS_NAMES[L.wt_dbg_suppress_logits(None, 1, 8, 8, pkg._fp(z), pkg._fp(z), None, 0, None, 0, 0)] == INVALID
    got = eng.dbg_suppress_logits(rows_of(1, 8, 1), [3])  # the engine is usable after each
    assert np.isneginf(got[0, 3])


# ---- a masked row behind the kernels that choose and score ----------------------------------------------------------

V, EOT, BEG = 8192, 4095, 4096  # the intervals' edges on a chunk boundary


def masked_case(eng, n_rows, seed, lists):
    """Rows of logits whose argmax, best timestamp and EOT are on the lists where `lists` says so; returns (z, masked by
    the kernel, always-list, first-list)."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n_rows, V)) * 2.0).astype(np.float32)
    always, first = lists(z)
    zp = np.zeros((n_rows, V + 8), np.float32)
    zp[:, :V] = z
    got = eng.dbg_suppress_logits(zp, always, first, True, V=V)[:, :V]
    want = np.stack([sup.filter_row(z[b], 0, always, first) for b in range(n_rows)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return z, np.ascontiguousarray(got), always, first


def id_rows(gs, stride=16):
    ids = np.zeros((len(gs), stride), np.int64)
    n = np.zeros(len(gs), np.int32)
    for b, g in enumerate(gs):
        ids[b, :N0] = PROMPT
        ids[b, N0:N0 + len(g)] = g
        n[b] = N0 + len(g)
    return ids, n


def test_timestamp_select_and_scores_behind_the_filter(eng):
    """ts_select and the score kernels on masked rows: the listed argmax is not chosen, rule 5 flips where the best text
    id is listed, and the log-probability's denominator leaves the listed ids out."""
    gs = [[BEG + 1, 5, 6], [BEG + 1, 5, 6], [BEG + 2, 7], [BEG + 1, 9, 10, 11]]

    def lists(z):
        # row 0: the best text id beats the timestamps' mass, the runner-up does not; both rows share the lists
        z[0, BEG:] -= 8.0
        z[0, 100] = 9.0
        z[0, BEG + 40] = 7.5
        z[0, :EOT][z[0, :EOT] > 5.0] = 5.0
        z[0, 100] = 9.0
        return sorted({100, int(np.argmax(z[1, :EOT])), int(BEG + np.argmax(z[2, BEG:]))}), [3]

    z, zm, always, first = masked_case(eng, len(gs), 21, lists)
    ids, n = id_rows(gs)
    tok, L, M = eng.dbg_timestamp_select(zm, ids, n, N0, EOT, BEG, 50)
    tok_plain, _, _ = eng.dbg_timestamp_select(z, ids, n, N0, EOT, BEG, 50)
    flipped = 0
    for b, g in enumerate(gs):
        want, info = ts_ref.step(zm[b], g, EOT, BEG, 50)
        assert min(info["gap_lm"], info["gap_top"]) > 1e-3
        assert int(tok[b]) == want and want not in always
        _, plain = ts_ref.step(z[b], g, EOT, BEG, 50)
        flipped += ("mass" in info["fired"]) != ("mass" in plain["fired"])
    assert flipped >= 1 and int(tok[0]) >= BEG and int(tok_plain[0]) == 100
    chosen = ids.copy()
    chosen[np.arange(len(gs)), n] = tok
    lp, _, _, den = eng.dbg_token_scores(zm, chosen, n + 1, N0, timestamps=True, eot=EOT, beg=BEG)
    for b, g in enumerate(gs):
        want_lp, want_den = scores_ref.token_logprob(zm[b], int(tok[b]), g, EOT, BEG, 50, True)
        assert abs(den[b] - want_den) < DEN_BOUND and abs(lp[b] - want_lp) < LP_BOUND


def test_plain_scores_rise_by_the_suppressed_mass(eng):
    """Filter before log-softmax: the chosen id's lp rises by exactly -log(1 - p_suppressed)."""
    def lists(z):
        z[:, 50] = 12.0  # a loud id that is listed, and a louder one that is chosen
        z[:, 60] = 13.0
        return [50, 0, V - 1], []

    z, zm, always, _ = masked_case(eng, 3, 22, lists)
    ids, n = id_rows([[5], [5, 6], [7, 8, 9]])
    chosen = ids.copy()
    chosen[np.arange(3), n] = 60
    lp_m, _, _, den_m = eng.dbg_token_scores(zm, chosen, n + 1, N0)
    lp_p, _, _, den_p = eng.dbg_token_scores(z, chosen, n + 1, N0)
    for b in range(3):
        p_sup = float(np.exp(z[b, always].astype(np.float64) - scores_ref.logsumexp64(z[b])).sum())
        assert p_sup > 0.1
        assert abs((lp_m[b] - lp_p[b]) + np.log1p(-p_sup)) < 2 * LP_BOUND
        assert abs(den_m[b] - scores_ref.logsumexp64(zm[b])) < DEN_BOUND


def test_the_sampler_never_draws_a_listed_id(eng):
    def lists(z):
        z[:, 50] = 12.0  # nearly all of the mass
        return [50], [int(np.argsort(z[0])[-2])]

    z, zm, always, first = masked_case(eng, 4, 23, lists)
    ids, n = id_rows([[], [], [], []])
    for T in (0.0, 0.6, 1.0):
        tok, _, _, key = eng.dbg_sample_select(zm, ids, n, N0, T, seed=5)
        for b in range(4):
            want, info = sample_ref.step(zm[b], [], T, seed=5, pos=N0 - 1, clip=b)
            assert int(tok[b]) == want and want != 50
        if T == 0.0:  # the greedy step of a suppressed plain decode: select_token's rule on the masked row
            assert [int(t) for t in tok] == [int(len(zm[b]) - 1 - np.argmax(zm[b][::-1])) for b in range(4)]
    assert int(eng.dbg_sample_select(zm, ids, n, N0, 0.0)[0][0]) != first[0]
    assert int(eng.dbg_sample_select(z, ids, n, N0, 0.0)[0][0]) == 50


def test_every_text_id_but_eot_listed(eng):
    """A -inf entry is outside every allowed set: with every text id listed, EOT and the timestamps are all that is left."""
    rng = np.random.default_rng(24)
    Vs, eot, beg = 1300, 1000, 1001
    z = (rng.standard_normal((2, Vs + 4)) * 2.0).astype(np.float32)
    z[:, beg:] -= 30.0  # the timestamps' mass stays below EOT's logit
    always = list(range(eot))
    zm = np.ascontiguousarray(eng.dbg_suppress_logits(z, always, [], False, V=Vs)[:, :Vs])
    gs = [[beg + 1, 5], [beg + 1, 5, 6]]
    ids, n = id_rows(gs)
    tok, _, M = eng.dbg_timestamp_select(zm, ids, n, N0, eot, beg, 50)
    assert [int(t) for t in tok] == [eot, eot] and np.array_equal(M, zm[:, eot])
    tok, _, _, _ = eng.dbg_sample_select(zm, ids, n, N0, 0.8, seed=2, timestamps=True, eot=eot, beg=beg)
    assert all(int(t) >= eot for t in tok)
    chosen = ids.copy()
    chosen[np.arange(2), n] = eot
    lp, _, _, den = eng.dbg_token_scores(zm, chosen, n + 1, N0, timestamps=True, eot=eot, beg=beg)
    for b in range(2):
        want_lp, want_den = scores_ref.token_logprob(zm[b], eot, gs[b], eot, beg, 50, True)
        assert abs(den[b] - want_den) < DEN_BOUND and abs(lp[b] - want_lp) < LP_BOUND


@pytest.mark.parametrize("timestamps", [False, True])
def test_a_beam_step_behind_the_filter(pkg, eng, timestamps):
    """beam_full_step on masked rows against beam_full_ref: a hypothesis whose allowed set the list shrinks below K + 1
    offers fewer ids, and no listed id is offered."""
    K, clips, cap = 4, 2, 12
    rng = np.random.default_rng(25)
    ch = Chain(pkg, K, clips, cap, V, EOT, BEG, timestamps, mit=-1, seed=3)
    gs = [[BEG + 1, 5, 6]] * (K * clips) if timestamps else [[3, 5, 6]] * (K * clips)
    z = (rng.standard_normal((K * clips, V)) * 2.0).astype(np.float32)
    keep = [7, 4094, EOT]  # row 0: three ids of its set are left
    always = [i for i in range(EOT) if i not in keep[:2]]
    if timestamps:
        z[0, BEG:] -= 40.0  # (rule 5 stays with the text, and the timestamps offer nothing that ranks)
    always_small = sorted({int(np.argmax(z[r, :EOT])) for r in range(1, K * clips)})
    zp = np.zeros((K * clips, V + 8), np.float32)
    zp[:, :V] = z
    zm = zp.copy()
    row0 = zp[:1]
    for lo in range(0, len(always), 1024):  # a list holds at most 1024 ids: four launches leave row 0 three text ids
        row0 = eng.dbg_suppress_logits(row0, always[lo: lo + 1024], [], False, V=V)
    zm[:1] = row0
    zm[1:] = eng.dbg_suppress_logits(zp[1:], always_small, [], False, V=V)
    zm = np.ascontiguousarray(zm[:, :V])
    n_live, n_fin = [K, K], [0, 0]
    sums = [[-0.1 * s for s in range(K)] for _ in range(clips)]
    ch.state["n_live"][:clips], ch.state["n_fin"][:clips] = n_live, n_fin
    ch.state["live_sum"][:clips, :K] = sums
    ids, lp, anc = ch.rows(gs)
    want = ch.expect(zm, gs, sums, n_live, n_fin)
    out = ch.step(eng, zm, gs, ids, lp, anc)
    ch.check(out, want, gs, ids, lp, anc, sums)
    lp0, _ = bfr.step_lp(zm[0], gs[0], EOT, BEG, timestamps, -1)
    if not timestamps:
        assert np.isfinite(lp0).sum() == len(keep) + (V - EOT - 1) and len(keep) < K + 1
    listed = set(always_small)
    assert not {int(t) for r, t in enumerate(out["token"]) if out["parent"][r] != 0} & listed
    for r in range(K * clips):
        lse = scores_ref.logsumexp64(zm[r][np.isfinite(bfr.step_lp(zm[r], gs[r], EOT, BEG, timestamps, -1)[0])])
        assert abs(out["lse"][r] - lse) < LSE_BOUND
