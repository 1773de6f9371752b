"""The kernels of full-length beam search (k_beam_full.hip) through their debug taps against
tests/beam_full_ref.py on hand-set tables: one step = beam_full_partial, beam_full_select, beam_full_advance (with
beam_full_begin in front where the step is a chain's first), and beam_full_finalize.  Without the feature the taps do
not exist and every test here fails."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_full_ref as bfr  # noqa: E402

pytestmark = pytest.mark.gpu

DELTA = 2e-4
# logsumexp_A against float64 numpy: the largest error measured over logits of scales 1, 30 and 300 is 1.72e-7 (8.4e-8,
# 1.72e-7 and 4.6e-8; the chunk sums are fp32 sums of 4096 expf values, merged in float64); the bound is five times that,
# far below DELTA / 2.  Sums are float64 and held to it; a log-probability is stored as a float32, so it carries half an
# ulp of a float32 below 64 (2^-19) on top
LSE_BOUND = 8.6e-7
LP_BOUND = LSE_BOUND + 2.0 ** -19
PROMPT = [7, 8, 9]
N0 = len(PROMPT)


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def state_of(g, beg):
    """The TsState of a hypothesis that generated g: tick of the last timestamp, g[-1] and g[-2] are timestamps."""
    stamps = [i for i in g if i >= beg]
    return [stamps[-1] - beg if stamps else -1, int(len(g) >= 1 and g[-1] >= beg), int(len(g) >= 2 and g[-2] >= beg)]


class Chain:
    """A step's inputs in the engine's layout (row = k * clips + c) next to the hypotheses they stand for."""

    def __init__(self, pkg, K, clips, cap, V, eot, beg, timestamps, mit=-1, c0=0, seed=0):
        self.pkg, self.K, self.clips, self.cap, self.V = pkg, K, clips, cap, V
        self.eot, self.beg, self.ts, self.mit, self.c0 = eot, beg, timestamps, mit, c0
        self.rng = np.random.default_rng(seed)
        self.state = pkg.beam_full_state(cap + 1)

    def rows(self, gs, lps=None):
        """ids / lp / anc rows of the hypotheses gs (one list of generated ids per row, equal lengths)."""
        n, t = len(gs), len(gs[0])
        ids = np.zeros((n, self.cap + 1), np.int64)
        lp = np.zeros((n, self.cap + 1), np.float32)
        ids[:, :N0] = PROMPT
        for r, g in enumerate(gs):
            ids[r, N0:N0 + t] = g
            lp[r, N0:N0 + t] = -self.rng.random(t) if lps is None else lps[r]
        anc = self.rng.integers(0, n, size=(n, self.cap)).astype(np.uint8)
        if self.ts:
            self.state["ts_state"][:n] = [state_of(g, self.beg) for g in gs]
        return ids, lp, anc

    def expect(self, logits, gs, sums, n_live, n_fin):
        """The reference's step per clip: dict(parent, token, lp, sum [K], n_live, n_fin, done, appended [(at, slot, lp, score)])."""
        K, clips, out = self.K, self.clips, []
        for c in range(clips):
            cands = []
            for s in range(n_live[c]):
                row = s * clips + c
                lp, _ = bfr.step_lp(logits[row], gs[row], self.eot, self.beg, self.ts, self.mit)
                for r, tok in enumerate(bfr.offered(lp, K)[:K + 1]):
                    cands.append((sums[c][s] + lp[tok], s, r, tok, float(lp[tok])))
            cands.sort(key=lambda x: (-x[0], x[1], x[2]))
            nf, live, app = n_fin[c], [], []
            for sc, s, _r, tok, lp in cands:
                if len(live) == K:
                    break
                if tok == self.eot:
                    if nf < K:
                        app.append((nf, s, lp, sc))
                        nf += 1
                else:
                    live.append((sc, s, tok, lp))
            out.append({"live": live, "n_fin": nf, "done": int(nf >= K or not live), "appended": app})
        return out

    def step(self, eng, logits, gs, ids, lp, anc, begin=False, **kw):
        t = len(gs[0])
        return eng.dbg_beam_full_step(self.state, logits, ids, lp, anc, K=self.K, clips=self.clips, pos=N0 - 1 + t, n_prompt=N0,
                                      cap=self.cap, eot=self.eot, beg=self.beg, timestamps=self.ts, max_initial=self.mit,
                                      c0=self.c0, begin=begin, **kw)

    def check(self, out, want, gs, ids, lp, anc, sums):
        """Everything a step writes against the reference's step."""
        K, clips, c0, t = self.K, self.clips, self.c0, len(gs[0])
        pos, st = N0 - 1 + t, self.state
        for c, w in enumerate(want):
            g_ = c0 + c
            nl = len(w["live"])
            assert st["n_live"][g_] == nl and st["n_fin"][g_] == w["n_fin"] and st["done"][g_] == w["done"], (c, w)
            for at, s, lp_eot, sc in w["appended"]:
                src = s * clips + c
                assert st["fin_len"][g_, at] == t + 1 and abs(st["fin_sum"][g_, at] - sc) < LSE_BOUND
                assert list(st["fin_tok"][g_, at, :t + 1]) == gs[src] + [self.eot]
                assert np.array_equal(st["fin_lp"][g_, at, :t], lp[src, N0:N0 + t]) and abs(st["fin_lp"][g_, at, t] - lp_eot) < LP_BOUND
            for k in range(K):
                row = k * clips + c
                if nl == 0:
                    assert out["parent"][row] == c and out["token"][row] == self.eot and st["live_sum"][g_, k] == -np.inf
                    continue
                sc, s, tok, lp_tok = w["live"][k if k < nl else 0]  # a missing slot follows the clip's slot 0
                par = s * clips + c
                assert out["parent"][row] == par and out["token"][row] == tok, (c, k, out["parent"][row], par, out["token"][row], tok)
                assert abs(lp_tok) < 64 and abs(out["tok_lp"][row] - lp_tok) < LP_BOUND
                if k < nl:
                    assert abs(st["live_sum"][g_, k] - sc) < LSE_BOUND
                else:
                    assert st["live_sum"][g_, k] == -np.inf
                # advance: the parent's rows, the token appended, anc[row][pos] = parent, nothing behind it
                assert list(out["ids_next"][row, :pos + 2]) == list(ids[par, :pos + 1]) + [tok] and (out["ids_next"][row, pos + 2:] == -7).all()
                assert np.array_equal(out["lp_next"][row, :pos + 1], lp[par, :pos + 1]) and out["lp_next"][row, pos + 1] == out["tok_lp"][row]
                assert (out["lp_next"][row, pos + 2:] == -7).all()
                assert np.array_equal(out["anc_next"][row, :pos], anc[par, :pos]) and out["anc_next"][row, pos] == par
                assert (out["anc_next"][row, pos + 1:] == 251).all()
                if self.ts:
                    assert list(st["ts_state"][row]) == state_of(gs[par] + [tok], self.beg), (c, k)


def histories(beg, t, n, rng):
    """n generated-id rows of length t >= 4 that end in text, in a closed pair, in one timestamp behind text, or in text
    behind a pair — the four states the rules tell apart."""
    kinds = [lambda: [beg + 1, 2, 3, 4], lambda: [beg + 1, 2, beg + 2, beg + 2], lambda: [beg + 1, 2, 3, beg + 3],
             lambda: [beg + 0, 2, beg + 1, beg + 1]]
    out = []
    for r in range(n):
        tail = kinds[r % 4]()
        out.append([beg + 0] + [1 + int(x) for x in rng.integers(0, 4, size=t - 5)] + tail if t > 4 else tail)
    return out


# V and the interval edges: eot / beg at, before and behind the 4096-entry chunk boundaries
EDGES = [(4101, 4090, 4096), (4101, 4094, 4095), (4101, 4095, 4097), (8192, 4095, 4096), (8192, 8000, 8188),
         (51865, 50257, 50364), (51865, 8191, 8192), (51865, 12287, 49152)]


@pytest.mark.parametrize("V,eot,beg", EDGES)
@pytest.mark.parametrize("timestamps", [True, False])
def test_a_step_against_the_reference(eng, pkg, V, eot, beg, timestamps):
    K, clips, cap, t = 4, 3, 40, 6
    ch = Chain(pkg, K, clips, cap, V, eot, beg, timestamps, seed=V + beg)
    rows = K * clips
    gs = histories(beg, t, rows, ch.rng) if timestamps else [[int(x) for x in ch.rng.integers(0, eot, size=t)] for _ in range(rows)]
    logits = (3.0 * ch.rng.standard_normal((rows, V))).astype(np.float32)
    logits[:, eot] += 6.0            # EOT competes
    logits[:, beg:beg + 12] += 5.0   # and so do the first timestamps, on both sides of rule 5
    logits[1, beg + 6:beg + 12] += 4.0
    logits[2, 5], logits[2, 9] = 11.0, 11.0    # a tie: the larger id first
    logits[3, 3], logits[3, 4] = -0.0, 0.0      # one value
    ids, lp, anc = ch.rows(gs)
    sums = -ch.rng.random((clips, 8)) * 3
    n_live, n_fin = [4, 3, 2], [0, 2, 3]
    logits[3 * clips + 1] = np.nan   # rows of missing slots are never read
    logits[2 * clips + 2] = np.nan
    logits[3 * clips + 2] = np.nan
    ch.state["n_live"][:clips], ch.state["n_fin"][:clips] = n_live, n_fin
    ch.state["live_sum"][:clips] = sums
    want = ch.expect(logits, gs, sums, n_live, n_fin)
    out = ch.step(eng, logits, gs, ids, lp, anc)
    ch.check(out, want, gs, ids, lp, anc, sums)
    for c in range(clips):  # logsumexp_A of the live rows, and the untouched entries of the others
        for s in range(K):
            row = s * clips + c
            if s < n_live[c]:
                lpr, _ = bfr.step_lp(logits[row], gs[row], eot, beg, timestamps)
                tok = int(np.argmax(lpr))
                assert abs(out["lse"][row] - (float(logits[row, tok]) - lpr[tok])) < LSE_BOUND
            else:
                assert out["lse"][row] == -7.0


def test_rule5_both_ways_and_the_partial_records(eng, pkg):
    V, eot, beg, K = 8192, 4000, 4100, 3
    ch = Chain(pkg, K, 1, 40, V, eot, beg, True)
    gs = [[beg + 1, 2, 3, 4]] * 3
    z = np.full((3, V), -9.0, np.float32)
    z[:, 10], z[:, 11], z[:, eot] = 2.0, 1.0, 0.5
    z[0, beg + 2:beg + 40] = 0.0    # L = log(38) = 3.64 > 2: only timestamps are offered, none of them above the text
    z[1, beg + 2:beg + 6] = 0.0     # L = log(4) = 1.39 < 2: text stays
    z[2] = -np.inf                  # a row of -inf offers nothing
    ids, lp, anc = ch.rows(gs)
    ch.state["n_live"][0] = 3
    sums = np.zeros((1, 8))
    sums[0, 1] = -2.5  # (so that both hypotheses reach the next step)
    ch.state["live_sum"][0] = sums[0]
    out = ch.step(eng, z, gs, ids, lp, anc, want_part=True)
    want = ch.expect(z, gs, sums, [3], [0])
    ch.check(out, want, gs, ids, lp, anc, sums)
    toks = {(int(out["parent"][k]), int(out["token"][k])) for k in range(K)}
    assert any(p == 0 and t >= beg for p, t in toks) and any(p == 1 and t in (10, 11) for p, t in toks)
    assert not any(p == 2 for p, _ in toks) and math.isnan(out["lse"][2])
    # the records: chunk 0 holds the text class, chunk 1 the timestamps (beg = 4100 lies 4 entries behind the boundary)
    st, keys = out["part_stats"], out["part_keys"]
    assert st[0, 0, 0] == 2.0 and st[0, 0, 2] == -np.inf and st[0, 1, 0] == -np.inf and st[0, 1, 2] == 0.0
    # (38 timestamps at 0 and the other V - beg - 40 allowed ones at -9)
    assert st[0, 1, 3] == pytest.approx(38.0 + (V - beg - 40) * math.exp(-9.0), rel=1e-6) and st[0, 0, 3] == 0.0
    assert [int(k) & 0xffffffff for k in keys[0, 0, 0, :3]] == [10, 11, eot] and not keys[0, 0, 1].any()
    assert [int(k) & 0xffffffff for k in keys[0, 1, 1, :3]] == [beg + 39, beg + 38, beg + 37] and not keys[0, 1, 0].any()
    assert (st[2, :, [0, 2]] == -np.inf).all() and not keys[2].any()


@pytest.mark.parametrize("mit,K,clips", [(0, 4, 3), (1, 4, 3), (3, 4, 3), (1, 2, 1), (7, 8, 3)])
def test_the_first_step_offers_what_a_holds(eng, pkg, mit, K, clips):
    """A of 1, 2 and K ids behind beam_full_begin: max_initial + 1 timestamps are allowed, so that many hypotheses live.
    The first step has one live row per clip: 1 and 3 rows."""
    V, eot, beg = 4101, 4000, 4050
    ch = Chain(pkg, K, clips, 40, V, eot, beg, True, mit=mit, c0=5)
    gs = [[]] * clips
    z = (3.0 * ch.rng.standard_normal((clips, V))).astype(np.float32)
    ids, lp, anc = ch.rows(gs)
    for v in ch.state.values():  # begin overwrites what an earlier chain left
        v[...] = 3
    ch.state["ts_state"][...] = 9
    out = ch.step(eng, z, gs, ids, lp, anc, begin=True)
    ids0, lp0, anc0 = ids, lp, anc.copy()
    anc0[:, :N0] = np.arange(clips)[:, None]  # begin: the prompt's K / V sit in the clip's own row
    sums = np.zeros((clips, 8))
    want = ch.expect(z, gs, sums, [1] * clips, [0] * clips)
    ch.check(out, want, gs, ids0, lp0, anc0, sums)
    assert all(len(w["live"]) == min(K, mit + 1) for w in want)
    assert (ch.state["n_live"][:5] == 3).all() and (ch.state["n_live"][5 + clips:] == 3).all()  # other clips' state stays


@pytest.mark.parametrize("K,clips", [(2, 1), (8, 16), (2, 64)])
def test_rows_1_to_128_and_finished_lists_of_160_ids(eng, pkg, K, clips):
    """Step t = 159 of K * clips rows: EOT wins in every clip, so finished entries of 160 ids are copied."""
    V, eot, beg, cap, t = 4101, 4000, 4050, 200, 159
    ch = Chain(pkg, K, clips, cap, V, eot, beg, False, seed=K * clips)
    rows = K * clips
    gs = [[int(x) for x in ch.rng.integers(0, eot, size=t)] for _ in range(rows)]
    z = (2.0 * ch.rng.standard_normal((rows, V))).astype(np.float32)
    for c in range(0, clips, 2):  # even clips: EOT tops every live row; odd clips: it is one id among 4101
        z[c::clips, eot] = 30.0
    ids, lp, anc = ch.rows(gs)
    sums = -ch.rng.random((clips, 8)) * 5
    ch.state["n_live"][:clips] = K
    ch.state["n_fin"][:clips] = [c % K for c in range(clips)]
    ch.state["live_sum"][:clips] = sums
    want = ch.expect(z, gs, sums, [K] * clips, [c % K for c in range(clips)])
    out = ch.step(eng, z, gs, ids, lp, anc)
    ch.check(out, want, gs, ids, lp, anc, sums)
    assert all(w["done"] == (c % 2 == 0) and bool(w["appended"]) == (c % 2 == 0) for c, w in enumerate(want))
    # a clip that is done keeps its rows behind themselves at the next step and changes nothing
    before = {k: v.copy() for k, v in ch.state.items()}
    gs2 = [g + [1] for g in gs]
    ids2, lp2, anc2 = ch.rows(gs2)
    out2 = ch.step(eng, z, gs2, ids2, lp2, anc2)
    for c, w in enumerate(want):
        if w["done"]:
            for k in range(K):
                row = k * clips + c
                assert out2["parent"][row] == row and out2["token"][row] == eot
            for name in ("n_fin", "n_live", "done", "fin_len", "fin_sum", "fin_tok", "fin_lp"):
                assert np.array_equal(ch.state[name][c], before[name][c]), name


def test_finalize_fills_ranks_and_copies(eng, pkg):
    K, clips, cap, t, eot = 4, 3, 200, 159, 4000
    ch = Chain(pkg, K, clips, cap, 4101, eot, 4050, False, c0=2, seed=4)
    rows = K * clips
    gs = [[int(x) for x in ch.rng.integers(0, eot, size=t + 1)] for _ in range(rows)]  # the rows after the last advance
    ids, lp, _ = ch.rows(gs)
    st = ch.state
    # clip 0: done with 4 finished entries, entries 1 and 3 tie on sum / len — the earlier one wins
    st["done"][2], st["n_fin"][2], st["n_live"][2] = 1, 4, 2
    st["fin_len"][2, :4] = [10, 5, 160, 10]
    st["fin_sum"][2, :4] = [-9.0, -2.0, -80.0, -4.0]
    st["fin_tok"][2, 1, :5], st["fin_lp"][2, 1, :5] = [11, 12, 13, 14, eot], [-0.25, -0.5, -0.25, -0.5, -0.5]
    # clip 1: 1 finished, 2 live -> 3 entries; the second live row has the best mean
    st["n_fin"][3], st["n_live"][3] = 1, 2
    st["fin_len"][3, 0], st["fin_sum"][3, 0] = 4, -4.0
    st["live_sum"][3, :2] = [-200.0, -100.0]
    # clip 2: nothing finished, 4 live, the long list of 160 ids: slot 0 wins a tie with slot 2
    st["n_live"][4] = 4
    st["live_sum"][4, :4] = [-50.0, -60.0, -50.0, -70.0]
    out = eng.dbg_beam_full_finalize(st, ids, lp, K=K, clips=clips, pos=N0 - 1 + t, n_prompt=N0, cap=cap, c0=2)
    assert list(out["out_len"][2:5]) == [5, t + 1, t + 1] and list(out["out_n"][2:5]) == [N0 + 5, N0 + t + 1, N0 + t + 1]
    assert list(out["out_sum"][2:5]) == [-2.0, -100.0, -50.0]
    assert list(out["out_ids"][2, :N0 + 5]) == PROMPT + [11, 12, 13, 14, eot] and not out["out_ids"][2, N0 + 5:].any()
    assert list(out["out_lp"][2, :N0 + 5]) == [0, 0, 0, -0.25, -0.5, -0.25, -0.5, -0.5] and not out["out_lp"][2, N0 + 5:].any()
    assert list(out["out_ids"][3, :N0 + t + 1]) == PROMPT + gs[1 * clips + 1]
    assert np.array_equal(out["out_lp"][3, N0:N0 + t + 1], lp[1 * clips + 1, N0:N0 + t + 1])
    assert list(out["out_ids"][4, :N0 + t + 1]) == PROMPT + gs[0 * clips + 2]
    assert list(st["n_fin"][2:5]) == [4, 3, 4] and list(st["fin_len"][4, :4]) == [t + 1] * 4
    assert (out["out_n"][:2] == -7).all() and (out["out_n"][5:] == -7).all()  # other clips' results stay


@pytest.mark.parametrize("scale", [1.0, 30.0, 300.0])
def test_logsumexp_of_the_allowed_set(eng, pkg, scale):
    """logsumexp_A against float64 numpy, with and without timestamps, rule 5 either way."""
    V, eot, beg, K, clips = 51865, 50257, 50364, 4, 8
    rng = np.random.default_rng(int(scale))
    worst = 0.0
    for timestamps in (True, False):
        ch = Chain(pkg, K, clips, 40, V, eot, beg, timestamps, seed=int(scale))
        rows = K * clips
        gs = histories(beg, 6, rows, ch.rng)
        z = (scale * rng.standard_normal((rows, V))).astype(np.float32)
        z[::2, beg:] += np.float32(scale)  # every other row: the timestamps' mass wins
        ids, lp, anc = ch.rows(gs)
        ch.state["n_live"][:clips] = K
        out = ch.step(eng, z, gs, ids, lp, anc)
        for row in range(rows):
            lpr, _ = bfr.step_lp(z[row], gs[row], eot, beg, timestamps)
            tok = int(np.argmax(lpr))
            worst = max(worst, abs(out["lse"][row] - (float(z[row, tok]) - lpr[tok])))
    print(f"scale {scale}: largest |logsumexp_A - float64| {worst:.2e}")
    assert worst < LSE_BOUND < DELTA / 2


def test_launcher_refusals_return_a_status(eng, pkg):
    def status(K=4, clips=3, c0=0, eot=4000, beg=4050):
        rows = K * clips
        c = Chain(pkg, K, clips, 40, 4101, eot, beg, True, c0=c0)
        gs = [[beg + 1, 2, 3, 4]] * rows
        ids, lp, anc = c.rows(gs)
        c.state["n_live"][:] = min(K, 8)
        try:
            c.step(eng, np.zeros((rows, 4101), np.float32), gs, ids, lp, anc)
        except pkg.WtError as e:
            return str(e).split(":")[0]
        return "WT_OK"

    assert status(K=1) == "WT_ERR_INVALID_ARG"
    assert status(K=9) == "WT_ERR_INVALID_ARG"
    assert status(c0=62) == "WT_ERR_INVALID_ARG"
    assert status(eot=4050, beg=4000) == "WT_ERR_INVALID_ARG"
    assert status(beg=4101) == "WT_ERR_INVALID_ARG"
    assert status() == "WT_OK"  # the engine is unharmed
