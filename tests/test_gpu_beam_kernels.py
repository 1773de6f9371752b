"""GPU (-m gpu): the beam-search kernels of csrc/k_beam.hip one by one, through the debug taps of include/wt_debug.h
(wt_dbg_beam_*), against numpy / float64 and tests/beam_ref.py.  Unlike tests/test_gpu_beam.py, whose model logits
never tie, these tests plant exact ties of every kind DESIGN section 11 orders (equal logits, equal scores across
slots and ranks, EOT candidates past a full list, equal sum / n_gen), vocabulary sizes at and around the 4096-entry
chunk boundary, signed zeros and -inf entries."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_ref  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 4096  # kBeamChunk: vocabulary entries per top-k block, 256 threads x 16 entries (thread t: t + 256 j)
U = 2.0 ** -24  # fp32 unit roundoff
INVALID = 1
# a chunk's s: 16 sequential adds per thread, a 6-level wave butterfly and 3 adds across the waves (25 roundings of a
# sum of positive terms: <= 25 U relative), expf within 4 ulps, and the rounding of z - m (|x| U relative on exp(x));
# doubled
S_ULPS = 2 * (25 + 4)


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def key_ids(keys):
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ top-k records ---
def topk_rows(V, rows, kk, ldl, seed):
    """rows x ldl logits: random rows and rows with planted ties, signed zeros, -inf entries and chunks, 1e4 values."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((rows, ldl)) * 3.0).astype(np.float32)
    z[:, V:] = np.nan  # past V: never read
    top = np.float32(20.0)
    planted = []

    def plant(fn):
        if len(planted) < rows:
            r = len(planted)
            fn(z[r])
            planted.append(r)

    c_last = (V - 1) // CHUNK

    def in_thread(row):  # entries t and t + 3 * 256 of one chunk: one thread's registers
        for c in range(c_last + 1):
            t = 37
            ids = [c * CHUNK + t, c * CHUNK + t + 3 * 256]
            if ids[1] < V:
                row[ids] = top

    def across_waves(row):  # threads 5 (wave 0), 70 (wave 1), 200 (wave 3)
        for c in range(c_last + 1):
            ids = [i for i in (c * CHUNK + 5, c * CHUNK + 70, c * CHUNK + 200) if i < V]
            row[ids] = top

    def chunk_boundary(row):
        row[[i for i in (CHUNK - 1, CHUNK) if i < V]] = top

    def kk_boundary(k):  # ranks k - 1 and k of every chunk tie (a ladder above them)
        def f(row):
            for c in range(c_last + 1):
                lo, hi = c * CHUNK, min(V, (c + 1) * CHUNK)
                ids = rng.choice(np.arange(lo, hi), size=min(hi - lo, k + 2), replace=False)
                vals = top - np.arange(ids.size, dtype=np.float32)
                vals[k:] = vals[k - 1] if k < ids.size else vals[k:]
                row[ids] = vals
        return f

    def signed_zeros(row, first_neg):
        row[:V] = -np.abs(row[:V]) - 1.0
        for c in range(c_last + 1):
            lo, hi = c * CHUNK, min(V, (c + 1) * CHUNK)
            if hi - lo >= 2:
                a, b = lo + (hi - lo) // 3, hi - 1
                row[a], row[b] = (np.float32(-0.0), np.float32(0.0)) if first_neg else (np.float32(0.0), np.float32(-0.0))

    def minus_inf(row):
        row[rng.choice(V, size=max(1, V // 7), replace=False)] = -np.inf

    def masked_chunk(row):
        c = min(1, c_last)
        row[c * CHUNK:min(V, (c + 1) * CHUNK)] = -np.inf
        if c_last == 0:  # one chunk: keep kk finite entries
            row[rng.choice(V, size=min(V, kk + 1), replace=False)] = 1.0

    def large(row):
        row[:V] = np.float32(1e4) + row[:V] * np.float32(0.5)

    for f in (in_thread, across_waves, chunk_boundary, kk_boundary(3), kk_boundary(5), kk_boundary(9),
              lambda r: signed_zeros(r, False), lambda r: signed_zeros(r, True), minus_inf, masked_chunk, large):
        plant(f)
    return z


def topk_ref(z, V, kk):
    """Per chunk: max, float64 sum of exp(z - max), top kk ids by (logit, larger id), from np.lexsort on the fp32 values."""
    rows = z.shape[0]
    n_ch = (V + CHUNK - 1) // CHUNK
    m = np.zeros((rows, n_ch), np.float32)
    ids = np.zeros((rows, n_ch, kk), np.int64)
    n_ids = np.zeros(n_ch, np.int64)
    for c in range(n_ch):
        lo, hi = c * CHUNK, min(V, (c + 1) * CHUNK)
        zc = z[:, lo:hi]
        m[:, c] = zc.max(axis=1)
        col = np.broadcast_to(np.arange(lo, hi), zc.shape)
        order = np.lexsort((-col, -zc), axis=1)[:, :kk]
        n_ids[c] = order.shape[1]
        ids[:, c, :n_ids[c]] = lo + order
    return m, ids, n_ids


def s_check(z, V, m_gpu, s_gpu):
    """s against the float64 sum of exp(z - m) at the kernel's m, within the bound of S_ULPS (+ the z - m rounding)."""
    n_ch = m_gpu.shape[1]
    for c in range(n_ch):
        lo, hi = c * CHUNK, min(V, (c + 1) * CHUNK)
        zc = z[:, lo:hi].astype(np.float64)
        mc = m_gpu[:, c].astype(np.float64)[:, None]
        with np.errstate(invalid="ignore"):
            x = np.where(np.isneginf(zc), -np.inf, zc - mc)
        x = np.where(np.isneginf(mc), -np.inf, x)
        e = np.exp(x)
        ref = e.sum(axis=1)
        sub = (np.abs(np.where(np.isfinite(x), x, 0.0)) * e).sum(axis=1)  # (e = 0 where x = -inf)
        tol = S_ULPS * U * ref + U * sub + 1e-30
        assert np.all(np.abs(s_gpu[:, c] - ref) <= tol), (c, np.max(np.abs(s_gpu[:, c] - ref) / np.maximum(ref, 1e-30)))


V_LIST = [1024, 4095, 4096, 4097, 51864, 51865, 65536]


@pytest.mark.parametrize("V", V_LIST)
def test_topk_records(eng, V):
    rows = 128 if V <= 4097 else 40
    ldl = V + 3
    z = topk_rows(V, rows, 9, ldl, seed=V)
    m_ref, ids_ref, n_ids = topk_ref(z[:, :V], V, 9)
    recs = {}
    for kk in (3, 5, 9):
        m, s, keys = eng.dbg_beam_topk(z, V, kk)
        assert np.array_equal(m, m_ref), kk  # a maximum is exact (and -0 == +0)
        for c in range(m.shape[1]):
            n = min(kk, n_ids[c])
            assert np.array_equal(key_ids(keys[:, c, :n]), ids_ref[:, c, :n]), (kk, c)
            assert np.all(keys[:, c, n:] == 0)  # a chunk of fewer than kk entries: no key
            assert np.all(keys[:, c, 1:n] < keys[:, c, :n - 1])  # keys strictly descending
        s_check(z[:, :V], V, m, s)
        recs[kk] = (m, s, keys)
    # top 3 and top 5 are prefixes of top 9; m and s do not depend on kk (bitwise)
    for kk in (3, 5):
        assert np.array_equal(recs[kk][2], recs[9][2][:, :, :kk])
        assert np.array_equal(recs[kk][0].view(np.uint32), recs[9][0].view(np.uint32))
        assert np.array_equal(recs[kk][1].view(np.uint32), recs[9][1].view(np.uint32))
    # the merged logsumexp of the records (float64 merge) against the row's float64 logsumexp
    m, s, _ = recs[9]
    M = m.astype(np.float64).max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        lse = M[:, 0] + np.log((s * np.exp(np.where(np.isneginf(m), -np.inf, m - M))).sum(axis=1))
    for r in range(rows):
        zr = z[r, :V].astype(np.float64)
        Mr = zr.max()
        ref = Mr + np.log(np.exp(zr - Mr).sum())
        # the relative error of s becomes an absolute one on log s: <= S_ULPS U, plus the z - m rounding (|z| U)
        assert abs(lse[r] - ref) <= S_ULPS * U + 2 * U * np.abs(zr[np.isfinite(zr)]).max() + 1e-12, (r, lse[r], ref)


def test_topk_signed_zeros_and_masked_chunk(eng):
    """The two input classes the kernel once got wrong: -0 against +0 (one logit: the larger id first) and a chunk of
    -inf entries only (m = -inf, s = 0, not NaN)."""
    V = 3 * CHUNK
    z = np.full((2, V), -5.0, np.float32)
    z[0, 100], z[0, 200] = np.float32(-0.0), np.float32(0.0)  # +0 at the larger id
    z[1, 100], z[1, 200] = np.float32(0.0), np.float32(-0.0)  # -0 at the larger id: must still come first
    z[:, CHUNK:2 * CHUNK] = -np.inf
    m, s, keys = eng.dbg_beam_topk(z, V, 3)
    assert list(key_ids(keys[0, 0, :2])) == [200, 100] and list(key_ids(keys[1, 0, :2])) == [200, 100]
    assert keys[0, 0, 0] == keys[1, 0, 0]  # id 200 holds +0 in row 0 and -0 in row 1: one key
    assert (keys[0, 0, 0] >> np.uint64(32)) == (keys[0, 0, 1] >> np.uint64(32))  # and one logit with id 100
    assert np.all(np.isneginf(m[:, 1])) and np.all(s[:, 1] == 0.0)
    assert np.all(np.isfinite(s))


def test_topk_records_are_a_function_of_the_row_alone(eng):
    V = 51865
    rng = np.random.default_rng(5)
    z = topk_rows(V, 24, 9, V, seed=11)
    m0, s0, k0 = eng.dbg_beam_topk(z, V, 9)
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a  # noqa: E731
    # other row indices, other row counts, other neighbours
    perm = rng.permutation(24)
    m1, s1, k1 = eng.dbg_beam_topk(z[perm], V, 9)
    other = (rng.standard_normal((7, V)) * 50).astype(np.float32)
    for r in (0, 6, 10, 23):
        mixed = other.copy()
        mixed[3] = z[r]
        m2, s2, k2 = eng.dbg_beam_topk(mixed, V, 9)
        m3, s3, k3 = eng.dbg_beam_topk(z[r:r + 1], V, 9)
        for mm, ss, kk_, row in ((m2, s2, k2, 3), (m3, s3, k3, 0)):
            assert np.array_equal(bits(mm[row]), bits(m0[r])) and np.array_equal(bits(ss[row]), bits(s0[r]))
            assert np.array_equal(kk_[row], k0[r])
    assert np.array_equal(bits(m1), bits(m0[perm])) and np.array_equal(bits(s1), bits(s0[perm]))
    assert np.array_equal(k1, k0[perm])


def test_topk_refuses_bad_shapes(eng, pkg):
    z = np.zeros((2, 70000), np.float32)
    for V, kk, rows in ((65537, 3, 2), (1024, 10, 2), (1024, 1, 2)):
        with pytest.raises(pkg.WtError) as e:
            eng.dbg_beam_topk(z[:rows, :max(V, 1024)], V, kk)
        assert e.value.code == INVALID
    with pytest.raises(pkg.WtError) as e:
        eng.dbg_beam_topk(np.zeros((129, 64), np.float32), 64, 3)
    assert e.value.code == INVALID


# ------------------------------------------------------------------------------------------------- select rules ---
def sentinel_state(eng):
    st = eng.beam_state(7)
    st["done"][:] = 0
    return st


def ladder_row(V, vals, rest=-8.0):
    """A row with given exact logits at given ids ({id: value}), every other entry `rest`."""
    z = np.full(V, rest, np.float32)
    for i, v in vals.items():
        z[i] = v
    return z


def lp64(z):
    return beam_ref.log_softmax64(z)


def id_rows(n, n_prompt, pos, seed):
    rng = np.random.default_rng(seed)
    ids = np.zeros((n, 32), np.int64)
    ids[:, :pos + 1] = rng.integers(1, 1000, size=(n, pos + 1))
    ids[:, :n_prompt] = [17, 23, 29, 31][:n_prompt]
    return ids


def step_lse_tol(z, lse):
    # fp32 merge of <= 16 records (each s within S_ULPS U) and logf, M + log S and z - lse roundings
    return (S_ULPS + 32) * U * (1.0 + abs(lse) + np.abs(z[np.isfinite(z)]).max())


def test_select_ties_lower_slot_then_lower_rank(eng):
    K, clips, c0, n_prompt, pos, V, eot = 4, 3, 5, 2, 4, 4100, 50
    # one row for every slot: ids 4097 and 300 tie at the top (across the chunk boundary), then 7, 2000, 9
    z = ladder_row(V, {4097: 4.0, 300: 4.0, 7: 3.0, 2000: 2.0, 9: 1.0})
    logits = np.tile(z, (K * clips, 1))
    ids = id_rows(K * clips, n_prompt, pos, 1)
    st = sentinel_state(eng)
    sums = np.array([-1.0, -1.0, -1.5, -1.0], np.float32)  # exact in binary: slots 0, 1, 3 tie
    st["live_sum"][c0:c0 + clips, :K] = sums
    st["n_fin"][c0:c0 + clips] = 0
    before = {k: v.copy() for k, v in st.items()}
    parent, token, nxt = eng.dbg_beam_step(K, clips, c0, K, pos, n_prompt, eot, logits, ids, st)
    lp = lp64(z)
    for c in range(clips):
        rows = [k * clips + c for k in range(K)]
        # six candidates share the best score (slots 0, 1, 3 x ranks 0, 1): slot 0's two ranks, then slot 1's
        assert list(parent[rows]) == [c, c, clips + c, clips + c], c
        assert list(token[rows]) == [4097, 300, 4097, 300], c
        want = [-1.0 + lp[4097]] * 4
        assert np.all(np.abs(st["live_sum"][c0 + c, :K] - want) <= step_lse_tol(z, 4.0 - lp[4097])), c
        for k, r in enumerate(rows):
            p = parent[r]
            assert list(nxt[r, :pos + 1]) == list(ids[p, :pos + 1]) and nxt[r, pos + 1] == token[r]
            assert np.all(nxt[r, pos + 2:] == 0)
    # nothing finished; every other clip and every other slot untouched
    for k in ("fin_tok", "fin_sum", "fin_len", "n_fin", "done"):
        assert np.array_equal(st[k], before[k]), k
    outside = np.ones(64, bool)
    outside[c0:c0 + clips] = False
    assert np.array_equal(st["live_sum"][outside], before["live_sum"][outside])
    assert np.array_equal(st["live_sum"][c0:c0 + clips, K:], before["live_sum"][c0:c0 + clips, K:])


def test_select_eot_past_a_full_list_is_dropped(eng):
    K, clips, c0, n_prompt, pos, V, eot = 4, 2, 9, 3, 7, 9000, 77
    z = ladder_row(V, {eot: 6.0, 5000: 3.0, 12: 2.5, 8191: 2.0, 8192: 1.0})  # EOT first in every row
    logits = np.tile(z, (K * clips, 1))
    ids = id_rows(K * clips, n_prompt, pos, 2)
    st = sentinel_state(eng)
    st["live_sum"][c0:c0 + clips, :K] = [-2.0, -1.0, -1.0, -1.0]  # slots 1..3 tie above slot 0
    st["n_fin"][c0:c0 + clips] = K - 1
    before = {k: v.copy() for k, v in st.items()}
    parent, token, _ = eng.dbg_beam_step(K, clips, c0, K, pos, n_prompt, eot, logits, ids, st)
    lp = lp64(z)
    t = pos + 1 - n_prompt
    for c in range(clips):
        g = c0 + c
        assert st["n_fin"][g] == K and st["done"][g] == 1
        # exactly one EOT (slot 1's: the lowest of the tied slots) entered the list, at its last place
        src = clips + c
        assert list(st["fin_tok"][g, K - 1, :t]) == list(ids[src, n_prompt:pos + 1]) and st["fin_tok"][g, K - 1, t] == eot
        assert np.array_equal(st["fin_tok"][g, K - 1, t + 1:], before["fin_tok"][g, K - 1, t + 1:])
        assert st["fin_len"][g, K - 1] == t + 1
        assert abs(st["fin_sum"][g, K - 1] - (-1.0 + lp[eot])) <= step_lse_tol(z, 6.0 - lp[eot])
        assert np.array_equal(st["fin_sum"][g, :K - 1], before["fin_sum"][g, :K - 1])
        assert np.array_equal(st["fin_len"][g, :K - 1], before["fin_len"][g, :K - 1])
        # the live rows: the non-EOT candidates in walk order (slots 1, 2, 3 rank 1, then slot 1 rank 2)
        rows = [k * clips + c for k in range(K)]
        assert list(parent[rows]) == [clips + c, 2 * clips + c, 3 * clips + c, clips + c]
        assert list(token[rows]) == [5000, 5000, 5000, 12]
    outside = np.ones(64, bool)
    outside[c0:c0 + clips] = False
    for k in st:
        assert np.array_equal(st[k][outside], before[k][outside]), k


def test_select_done_clip_changes_nothing(eng):
    K, clips, c0, n_prompt, pos, V, eot = 3, 4, 1, 1, 5, 2048, 9
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((K * clips, V)).astype(np.float32)
    ids = id_rows(K * clips, n_prompt, pos, 3)
    st = sentinel_state(eng)
    st["n_fin"][c0:c0 + clips] = [0, K, 1, K]
    st["done"][c0:c0 + clips] = [0, 1, 0, 1]
    st["live_sum"][c0:c0 + clips, :K] = -1.0
    before = {k: v.copy() for k, v in st.items()}
    parent, token, nxt = eng.dbg_beam_step(K, clips, c0, K, pos, n_prompt, eot, logits, ids, st)
    for c in (1, 3):
        g = c0 + c
        rows = [k * clips + c for k in range(K)]
        assert list(parent[rows]) == rows and list(token[rows]) == [eot] * K
        for r in rows:
            assert list(nxt[r, :pos + 1]) == list(ids[r, :pos + 1]) and nxt[r, pos + 1] == eot
        for k in st:
            assert np.array_equal(st[k][g], before[k][g]), (k, c)
    for c in (0, 2):
        assert not np.array_equal(st["live_sum"][c0 + c], before["live_sum"][c0 + c])


def test_select_step0_layout_and_merged_lse(eng):
    """Step 0: one prompt row per clip (n_live = 1, sum 0); the new live sums are the lp of the K best tokens, whose
    fp32 logsumexp merges the chunk records with their own maxima (chunk maxima far apart)."""
    K, clips, c0, n_prompt, V, eot = 5, 25, 3, 4, 51865, 50257
    pos = n_prompt - 1
    rng = np.random.default_rng(4)
    logits = (rng.standard_normal((clips, V)) * 2.0).astype(np.float32)
    for c in range(clips):
        logits[c, (c % 13) * CHUNK:(c % 13 + 1) * CHUNK] += np.float32(6.0 + c % 5)  # one dominant chunk
        if c % 4 == 0:
            logits[c, eot] = logits[c].max() + 1.0  # EOT first: finishes at step 0 (t = 0: list of EOT alone)
    ids = id_rows(clips, n_prompt, pos, 4)
    st = sentinel_state(eng)
    st["n_fin"][c0:c0 + clips] = 0
    parent, token, nxt = eng.dbg_beam_step(K, clips, c0, 1, pos, n_prompt, eot, logits, ids, st)
    for c in range(clips):
        g = c0 + c
        z = logits[c]
        lp = lp64(z)
        order = [int(i) for i in beam_ref.ranked(lp, K + 1)]
        live = [i for i in order if i != eot][:K]
        rows = [k * clips + c for k in range(K)]
        assert list(parent[rows]) == [c] * K and list(token[rows]) == live, c
        lse = float(z.astype(np.float64)[order[0]] - lp[order[0]])
        assert np.all(np.abs(st["live_sum"][g, :K] - lp[live]) <= step_lse_tol(z, lse)), c
        if eot in order:
            assert st["n_fin"][g] == 1 and st["fin_len"][g, 0] == 1 and st["fin_tok"][g, 0, 0] == eot
            assert abs(st["fin_sum"][g, 0] - lp[eot]) <= step_lse_tol(z, lse)
        else:
            assert st["n_fin"][g] == 0
        for k, r in enumerate(rows):
            assert list(nxt[r, :pos + 1]) == list(ids[c, :pos + 1]) and nxt[r, pos + 1] == live[k]


# ------------------------------------------------------------------------------------------------------ reorder ---
@pytest.mark.parametrize("d", [64, 384, 512])
def test_reorder_copies_history_and_nothing_else(eng, d):
    cap, slabs, src_rows, dst_rows, V = 32, 3, 5, 12, 1000
    rng = np.random.default_rng(d)
    kv_src = rng.standard_normal((slabs, src_rows, cap, d)).astype(np.float32)
    ids_src = rng.integers(1, V, size=(src_rows, 32)).astype(np.int64)
    # permuted and duplicated parents, two out of range (clamped to 0 and src_rows - 1)
    parent = np.array([3, 0, 4, 4, 1, 2, 0, -3, 99, 2, 1, 3], np.int32)
    token = np.array([5, 999, 0, -1, 1000, 77, 12, 13, 14, 2 ** 40, 15, 16], np.int64)  # -1, 1000, 2^40: written as 0
    clamped = np.clip(parent, 0, src_rows - 1)
    tok_ok = np.where((token >= 0) & (token < V), token, 0)
    SENT = np.float32(-777.25)
    poses = range(31) if d == 64 else (0, 1, 16, 29, 30)
    for pos in poses:
        kv_dst = np.full((slabs * dst_rows + 1, cap, d), SENT, np.float32)
        ids_dst = np.full((128, 32), -5, np.int64)
        kv, idd = eng.dbg_beam_reorder(src_rows, dst_rows, cap, d, slabs, pos, V, kv_src, kv_dst, ids_src, ids_dst,
                                       parent, token)
        kv4 = kv[:slabs * dst_rows].reshape(slabs, dst_rows, cap, d)
        assert np.array_equal(kv4[:, :, :pos + 1], kv_src[:, clamped, :pos + 1]), pos
        assert np.all(kv4[:, :, pos + 1:] == SENT) and np.all(kv[slabs * dst_rows] == SENT), pos
        assert np.array_equal(idd[:dst_rows, :pos + 1], ids_src[clamped, :pos + 1]), pos
        assert np.array_equal(idd[:dst_rows, pos + 1], tok_ok), pos
        assert np.all(idd[:dst_rows, pos + 2:] == 0) and np.all(idd[dst_rows:] == -5), pos


def test_reorder_refuses_bad_shapes(eng, pkg):
    ids = np.zeros((4, 32), np.int64)
    for cap, d, pos in ((8, 64, 8), (8, 62, 2), (40, 64, 31)):  # pos + 1 > cap, d % 4, pos + 1 >= 32
        with pytest.raises(pkg.WtError) as e:
            eng.dbg_beam_reorder(4, 4, cap, d, 2, pos, 100, np.zeros((2, 4, cap, d), np.float32),
                                 np.zeros((2 * 4 + 1, cap, d), np.float32), ids, np.zeros((128, 32), np.int64),
                                 np.zeros(4, np.int32), np.zeros(4, np.int64))
        assert e.value.code == INVALID


# ----------------------------------------------------------------------------------------------------- finalize ---
def test_finalize_ties_fill_and_cap(eng):
    K, c0, n_prompt = 3, 6, 2
    clips = 3
    pos = 30  # max_pos = 31: the live rows hold t + 1 = 30 generated ids, n = 2 + 30 = 32; a longer entry stops at 32
    t = pos + 1 - n_prompt
    ids = id_rows(K * clips, n_prompt, pos + 1, 6)
    st = sentinel_state(eng)
    g0, g1, g2 = c0, c0 + 1, c0 + 2
    # clip 0 (done): -3/1, -2/1, -4/2: -2/1 and -4/2 tie, the earlier entry wins
    st["done"][g0], st["n_fin"][g0] = 1, K
    st["fin_sum"][g0, :K], st["fin_len"][g0, :K] = [-3.0, -2.0, -4.0], [1, 1, 2]
    st["fin_tok"][g0, 1, :1] = [333]
    # clip 1 (done): -4/2 first, then -2/1: the earlier (longer) entry wins
    st["done"][g1], st["n_fin"][g1] = 1, K
    st["fin_sum"][g1, :K], st["fin_len"][g1, :K] = [-4.0, -2.0, -9.0], [2, 1, 3]
    st["fin_tok"][g1, 0, :2] = [444, 445]
    # clip 2 (not done, one entry of length 31 -> n_prompt + 31 = 33 ids): the fill takes live slots 0 and 1
    st["done"][g2], st["n_fin"][g2] = 0, 1
    st["fin_sum"][g2, 0], st["fin_len"][g2, 0] = -62.0, 31
    st["fin_tok"][g2, 0, :31] = np.arange(500, 531)
    st["live_sum"][g2, :K] = [-29.0, -14.5, -1.0]  # slot 2 would be best, but the list is full after slot 1
    before = {k: v.copy() for k, v in st.items()}
    out = {"ids": np.full((64, 32), -9, np.int64), "n": np.full(64, -9, np.int32), "sum": np.full(64, -9, np.float32),
           "len": np.full(64, -9, np.int32)}
    out = eng.dbg_beam_finalize(K, clips, c0, pos, n_prompt, ids, st, out)
    prompt = list(ids[0, :n_prompt])
    assert out["sum"][g0] == -2.0 and out["len"][g0] == 1 and out["n"][g0] == n_prompt + 1
    assert list(out["ids"][g0, :n_prompt + 1]) == prompt + [333] and np.all(out["ids"][g0, n_prompt + 1:] == 0)
    assert out["sum"][g1] == -4.0 and out["len"][g1] == 2
    assert list(out["ids"][g1, :n_prompt + 2]) == prompt + [444, 445]
    for k in (0, 1):  # the fill: live slots 0 and 1 into places 1 and 2
        r = k * clips + 2
        assert list(st["fin_tok"][g2, 1 + k, :t + 1]) == list(ids[r, n_prompt:pos + 2])
        assert st["fin_sum"][g2, 1 + k] == st["live_sum"][g2, k] and st["fin_len"][g2, 1 + k] == t + 1
    assert st["n_fin"][g2] == K
    # -62/31, -29/30, -14.5/30: slot 1's row, 32 ids
    assert out["sum"][g2] == np.float32(-14.5) and out["len"][g2] == t + 1 and out["n"][g2] == 32
    assert list(out["ids"][g2]) == prompt + list(ids[clips + 2, n_prompt:pos + 2])
    # the capped case: the first entry alone at its 32 ids
    st2 = {k: v.copy() for k, v in before.items()}
    st2["live_sum"][g2, :K] = [-90.0, -90.0, -90.0]
    out2 = eng.dbg_beam_finalize(K, clips, c0, pos, n_prompt, ids, st2)
    assert out2["n"][g2] == 32 and out2["len"][g2] == 31
    assert list(out2["ids"][g2]) == prompt + list(range(500, 530))
    # every other clip's output and state untouched
    outside = np.ones(64, bool)
    outside[c0:c0 + clips] = False
    for k in ("ids", "n", "sum", "len"):
        assert np.all(out[k][outside] == -9), k
    for k in st:
        assert np.array_equal(st[k][outside], before[k][outside]), k


# --------------------------------------------------------------------------------- whole searches on table logits ---
DELTA = 2e-4  # decision margin: every decision gap of a table is 0 (a tie the rules decide) or above it
SUM_TOL = 1e-4  # |fp32 sum - float64 sum|: <= 31 steps of an lp (|lp| < 16) and a sum (|sum| < 200) rounded, ~2 ulps each


class Table:
    """Deterministic logits of a prefix, per clip, with no model: a shared background and a few hot entries whose ids
    and values are a function of the prefix's CLASSES (id // 2).  Hot entries come as pairs (ids 2j, 2j + 1, one
    value) or singles, so that siblings — hypotheses that differ only inside a pair — have bitwise-identical rows and
    sums from then on: every kind of tie happens.  EOT grows with the generated length, so clips finish."""

    def __init__(self, V, eot, seed, n_prompt, eot_rate):
        self.V, self.eot, self.seed, self.n_prompt, self.eot_rate = V, eot, seed, n_prompt, eot_rate
        rng = np.random.default_rng(seed)
        self.base = (rng.standard_normal(V) * 0.5 - 9.0).astype(np.float32)
        self.memo = {}

    def hot(self, clip, prefix):
        key = (clip,) + tuple(int(i) // 2 for i in prefix)
        if key not in self.memo:
            h = zlib.crc32(np.asarray(key, np.int64).tobytes()) ^ (self.seed << 8)
            rng = np.random.default_rng(h)
            n = 10
            cls = rng.choice(self.V // 2, size=n, replace=False)
            vals = (rng.integers(0, 360, size=n) * 0.025).astype(np.float32)  # on a grid: equal, or 0.025 apart
            mode = rng.integers(0, 3, size=n)  # 0: the pair, 1: the even id, 2: the odd id
            ids, v = [], []
            for c, x, md in zip(cls, vals, mode):
                for i in ((2 * c, 2 * c + 1) if md == 0 else (2 * c + md - 1,)):
                    if i < self.V and i != self.eot:
                        ids.append(int(i))
                        v.append(x)
            n_gen = len(prefix) - self.n_prompt
            e = np.float32(0.025 * np.round((rng.uniform(-1.0, 6.0) + self.eot_rate * n_gen) / 0.025))
            self.memo[key] = (np.asarray(ids), np.asarray(v, np.float32), e)
        return self.memo[key]

    def row(self, clip, prefix):
        ids, v, e = self.hot(clip, prefix)
        z = self.base.copy()
        z[ids] = v
        z[self.eot] = e
        return z

    def fn(self, clip):
        return lambda prefix: self.row(clip, prefix)


def gpu_search(eng, tab, K, clips, c0, prompt, max_pos, eot):
    """decode_beam's step loop through wt_dbg_beam_step over table logits, then wt_dbg_beam_finalize."""
    n_prompt = len(prompt)
    ids = np.zeros((clips, 32), np.int64)
    ids[:, :n_prompt] = prompt
    st = sentinel_state(eng)
    st["n_fin"][c0:c0 + clips] = 0
    before = {k: v.copy() for k, v in st.items()}
    for t in range(max_pos - n_prompt + 1):
        pos = n_prompt - 1 + t
        n_live = 1 if t == 0 else K
        logits = np.stack([tab.row(r % clips, list(ids[r, :pos + 1])) for r in range(n_live * clips)])
        _, _, ids = eng.dbg_beam_step(K, clips, c0, n_live, pos, n_prompt, eot, logits, ids, st)
    out = eng.dbg_beam_finalize(K, clips, c0, max_pos - 1, n_prompt, ids, st)
    outside = np.ones(64, bool)
    outside[c0:c0 + clips] = False
    for k in st:
        assert np.array_equal(st[k][outside], before[k][outside]), k
    return out


SEARCHES = [  # K, clips, c0, V, n_prompt, max_pos, eot_rate, seed
    (2, 62, 2, 4097, 3, 12, 0.5, 1),
    (4, 32, 0, 51865, 1, 31, 0.15, 1),  # one clip runs to max_pos: its list is filled from the live rows
    (5, 25, 7, 1024, 4, 20, 0.3, 1),
    (8, 16, 40, 51865, 2, 14, 0.4, 1),
]


@pytest.mark.parametrize("K,clips,c0,V,n_prompt,max_pos,eot_rate,seed", SEARCHES)
def test_whole_search_matches_the_reference(eng, K, clips, c0, V, n_prompt, max_pos, eot_rate, seed):
    eot = V - 7 if V > 4096 else 3
    prompt = [11, 13, 17, 19][:n_prompt]
    tab = Table(V, eot, seed, n_prompt, eot_rate)
    out = gpu_search(eng, tab, K, clips, c0, prompt, max_pos, eot)
    gaps = {k: [] for k in beam_ref.GAP_KINDS}
    dropped = 0
    for c in range(clips):
        r = beam_ref.beam_search(tab.fn(c), prompt, K, max_pos, eot)
        g = c0 + c
        got = [int(i) for i in out["ids"][g, :out["n"][g]]]
        assert got == r["ids"], (c, got, r["ids"])
        assert out["len"][g] == r["n_gen"], c
        assert abs(float(out["sum"][g]) - r["sum"]) <= SUM_TOL, (c, out["sum"][g], r["sum"])
        for k in beam_ref.GAP_KINDS:
            gaps[k] += r["gaps"][k]
        dropped += r["eot_dropped"]
    # the table exercised every tie rule, and no decision rested on a gap fp32 could flip
    for k in beam_ref.GAP_KINDS:
        a = np.asarray(gaps[k])
        assert np.any(a == 0.0), k
        assert np.all((a == 0.0) | (np.abs(a) > DELTA)), (k, np.abs(a[a != 0.0]).min())
    assert dropped > 0
