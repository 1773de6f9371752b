"""The ragged chain's kernels (wt_engine_set_contexts) through their debug taps: self_attention_long
and self_attention_prefill under a slot count with per-clip starts, the embedding prologue's pos_start and the position
cap.  A clip at Whisper position slot - start[b] carries the bits of the unragged tap at that position and meets float64
numpy over its own keys at the project's bar; a clip outside [0, P) is void: zeros out, caches untouched.  Without the
feature the taps do not exist and every test here fails."""
from ctypes import POINTER, c_float, c_int32

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 1e-5  # the project's bar for this computation (tests/test_gpu_self_attention_prefill.py)
INVALID = "WT_ERR_INVALID_ARG"
SLOTS = (0, 5, 31, 32, 63, 64, 65, 127, 159, 447)
worst = {"long": 0.0, "prefill": 0.0}


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()
    print("largest |delta| against float64: long %.2e, prefill %.2e" % (worst["long"], worst["prefill"]))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def attend64(q, k, v, H):
    """float64 attention of one query [d] over keys / values [n][d], per head."""
    out = np.zeros(64 * H)
    for h in range(H):
        sl = slice(64 * h, 64 * h + 64)
        s = (k[:, sl].astype(np.float64) @ q[sl].astype(np.float64)) / 8.0
        p = np.exp(s - s.max())
        out[sl] = (p / p.sum()) @ v[:, sl].astype(np.float64)
    return out


def caches(rng, B, cap, d, known, fill):
    """[B][cap][d] k and v: clip b's rows < known[b] standard normal, every other row `fill`."""
    kc = np.full((B, cap, d), fill, np.float32)
    vc = np.full((B, cap, d), fill, np.float32)
    for b in range(B):
        n = max(0, min(known[b], cap))
        kc[b, :n] = rng.standard_normal((n, d))
        vc[b, :n] = rng.standard_normal((n, d))
    return kc, vc


@pytest.mark.parametrize("H", [2, 6])
@pytest.mark.parametrize("cap", [160, 448])
@pytest.mark.parametrize("slot", SLOTS)
def test_long_kernel_per_clip_positions(eng, H, cap, slot):
    B, d = 3, 64 * H
    for starts in ((0, 5, slot), (0, slot + 1, 0)):
        for P in sorted({cap, min(max(slot, 1), cap)}):  # above the slot (where the cache allows it), and at it
            q = [slot - s for s in starts]
            live = [0 <= x < P for x in q]
            rng = np.random.default_rng([H, cap, slot, P, starts[1]])
            qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
            state = rng.bit_generator.state
            kc, vc = caches(rng, B, cap, d, [x if ok else 0 for x, ok in zip(q, live)], 1e30)
            out, k2, v2 = eng.dbg_self_attention_long_ragged(qkv, kc, vc, slot, starts, P)
            for b in range(B):
                if not live[b]:  # void: zeros, nothing appended
                    assert not out[b].any() and np.array_equal(bits(k2[b]), bits(kc[b])) and np.array_equal(bits(v2[b]), bits(vc[b]))
                    continue
                o1, k1, v1 = eng.dbg_self_attention_long(qkv[b:b + 1], kc[b:b + 1], vc[b:b + 1], q[b])
                assert np.array_equal(bits(out[b]), bits(o1[0])), (starts, P, b)
                assert np.array_equal(bits(k2[b]), bits(k1[0])) and np.array_equal(bits(v2[b]), bits(v1[0]))
                keys = np.concatenate([kc[b, :q[b]], qkv[b:b + 1, d:2 * d]])
                vals = np.concatenate([vc[b, :q[b]], qkv[b:b + 1, 2 * d:]])
                err = np.abs(out[b] - attend64(qkv[b, :d], keys, vals, H)).max()
                worst["long"] = max(worst["long"], err)
                assert err <= BAR, (starts, P, b, err)
            # the tails and the void clips' caches do not matter: zeros in their place give the same bits
            rng.bit_generator.state = state
            kz, vz = caches(rng, B, cap, d, [x if ok else 0 for x, ok in zip(q, live)], 0.0)
            outz, _, _ = eng.dbg_self_attention_long_ragged(qkv, kz, vz, slot, starts, P)
            assert np.array_equal(bits(outz), bits(out))
    if slot < cap:  # all starts 0: the unragged launch, bit for bit
        rng = np.random.default_rng([H, cap, slot])
        qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
        kc, vc = caches(rng, B, cap, d, [slot] * B, 1e30)
        got = eng.dbg_self_attention_long_ragged(qkv, kc, vc, slot, (0, 0, 0), cap)
        want = eng.dbg_self_attention_long(qkv, kc, vc, slot)
        assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def prefill_starts(B, pos0, n):
    """Start vectors that put a clip's position 0 before the launch's range, at its first slot, inside it (mid query group
    and on a 16-boundary), at its last slot and behind it — rotated over the clips."""
    choices = [0, max(pos0 - 7, 0), pos0, pos0 + 5, pos0 + 16, pos0 + n - 1, pos0 + n, pos0 + n + 9]
    return [tuple(choices[(i + b) % len(choices)] for b in range(B)) for i in range(len(choices))]


@pytest.mark.parametrize("B,pos0,n", [(1, 0, 128), (3, 0, 40), (3, 30, 20), (5, 224, 25)])
def test_prefill_kernel_per_clip_positions(eng, B, pos0, n):
    H, cap = 6, 448
    d = 64 * H
    for starts in prefill_starts(B, pos0, n):
        for P in sorted({cap, min(max(1, pos0 - min(starts) + n // 2), cap)}):  # the whole cache, and a cap inside the launch
            q0 = [pos0 - s for s in starts]
            lo = [max(0, -x) for x in q0]            # the first live query
            hi = [min(n, P - x) for x in q0]         # one past the last
            rng = np.random.default_rng([B, pos0, n, P] + list(starts))
            qkv = rng.standard_normal((n * B, 3 * d)).astype(np.float32)
            rows = qkv.reshape(n, B, 3 * d)
            state = rng.bit_generator.state
            known = [max(x, 0) if l < h else 0 for x, l, h in zip(q0, lo, hi)]
            kc, vc = caches(rng, B, cap, d, known, 1e30)
            out, k2, v2 = eng.dbg_self_attention_prefill_ragged(qkv, kc, vc, pos0, n, starts, P)
            out = out.reshape(n, B, d)
            for b in range(B):
                if lo[b] >= hi[b]:  # the whole clip is void
                    assert not out[:, b].any() and np.array_equal(bits(k2[b]), bits(kc[b])) and np.array_equal(bits(v2[b]), bits(vc[b]))
                    continue
                assert not out[:lo[b], b].any() and not out[hi[b]:, b].any()  # void queries next to live ones
                first = q0[b] + lo[b]
                o1, k1, v1 = eng.dbg_self_attention_prefill(np.ascontiguousarray(rows[lo[b]:hi[b], b]), kc[b:b + 1], vc[b:b + 1],
                                                            first, hi[b] - lo[b])
                assert np.array_equal(bits(out[lo[b]:hi[b], b]), bits(o1)), (starts, P, b)
                assert np.array_equal(bits(k2[b]), bits(k1[0])) and np.array_equal(bits(v2[b]), bits(v1[0]))
                keys = np.concatenate([kc[b, :first], rows[lo[b]:hi[b], b, d:2 * d]])
                vals = np.concatenate([vc[b, :first], rows[lo[b]:hi[b], b, 2 * d:]])
                for p in (lo[b], (lo[b] + hi[b]) // 2, hi[b] - 1):  # the first, a middle and the last live query
                    nk = q0[b] + p + 1
                    err = np.abs(out[p, b] - attend64(rows[p, b, :d], keys[:nk], vals[:nk], H)).max()
                    worst["prefill"] = max(worst["prefill"], err)
                    assert err <= BAR, (starts, P, b, p, err)
            rng.bit_generator.state = state
            kz, vz = caches(rng, B, cap, d, known, 0.0)
            outz, _, _ = eng.dbg_self_attention_prefill_ragged(qkv, kz, vz, pos0, n, starts, P)
            assert np.array_equal(bits(outz.reshape(n, B, d)), bits(out))
    # all starts 0: the unragged launch, bit for bit
    rng = np.random.default_rng([B, pos0, n])
    qkv = rng.standard_normal((n * B, 3 * d)).astype(np.float32)
    kc, vc = caches(rng, B, cap, d, [pos0] * B, 1e30)
    got = eng.dbg_self_attention_prefill_ragged(qkv, kc, vc, pos0, n, (0,) * B, cap)
    want = eng.dbg_self_attention_prefill(qkv, kc, vc, pos0, n)
    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def test_the_launchers_refuse_what_the_unragged_forms_refuse(eng, pkg):
    L = pkg.lib()
    fp = lambda a: a.ctypes.data_as(POINTER(c_float))  # noqa: E731

    def arrays(B, H, cap, n):
        Bc, Hc, capc, nc = max(B, 1), max(H, 1), max(min(cap, 448), 1), max(min(n, 128), 1)
        k = np.zeros((Bc, capc, Hc * 64), np.float32)
        return np.zeros((nc * Bc, 3 * Hc * 64), np.float32), k, k.copy(), np.zeros((nc * Bc, Hc * 64), np.float32), np.zeros(Bc, np.int32)

    def long_(B, H, cap, pos, P, start=True):
        q, k, v, o, s = arrays(B, H, cap, 1)
        sp = s.ctypes.data_as(POINTER(c_int32)) if start else None
        return pkg.STATUS_NAMES.get(L.wt_dbg_self_attention_long_ragged(eng.handle, B, H, cap, pos, fp(q), fp(k), fp(v), fp(o), sp, P))

    def prefill(B, H, cap, pos0, n, P, start=True):
        q, k, v, o, s = arrays(B, H, cap, n)
        sp = s.ctypes.data_as(POINTER(c_int32)) if start else None
        return pkg.STATUS_NAMES.get(L.wt_dbg_self_attention_prefill_ragged(eng.handle, B, H, cap, pos0, n, fp(q), fp(k), fp(v), fp(o), sp, P))

    assert long_(3, 2, 160, -1, 160) == INVALID
    assert long_(3, 2, 449, 10, 449) == INVALID
    assert long_(0, 2, 160, 10, 160) == INVALID
    assert long_(3, 0, 160, 10, 160) == INVALID
    assert long_(3, 2, 160, 10, 0) == INVALID      # no position to feed
    assert long_(3, 2, 160, 10, 161) == INVALID    # a limit past the cache
    assert long_(3, 2, 160, 896, 160) == INVALID   # a slot past twice the longest cache
    assert long_(3, 2, 160, 10, 160, start=False) == INVALID
    assert long_(3, 2, 160, 200, 160) == "WT_OK"   # a slot past the cache: every clip void
    assert prefill(3, 2, 160, -1, 4, 160) == INVALID
    assert prefill(3, 2, 160, 10, 0, 160) == INVALID
    assert prefill(3, 2, 160, 157, 4, 160) == INVALID
    assert prefill(3, 2, 449, 10, 4, 449) == INVALID
    assert prefill(3, 2, 448, 10, 43, 448) == INVALID  # 129 rows
    assert prefill(0, 2, 160, 40, 4, 160) == INVALID
    assert prefill(3, 0, 160, 40, 4, 160) == INVALID
    assert prefill(3, 2, 160, 40, 4, 0) == INVALID
    assert prefill(3, 2, 160, 40, 4, 161) == INVALID
    assert prefill(3, 2, 160, 40, 4, 160, start=False) == INVALID
    assert prefill(3, 2, 448, 406, 42, 448) == "WT_OK"


def test_a_wild_start_array_touches_nothing(eng):
    """Every index derived from the start array is bounded inside the kernels: starts far outside any chain make void
    clips, whatever they hold."""
    H, B, cap = 2, 3, 160
    d = 64 * H
    rng = np.random.default_rng(11)
    wild = (-2 ** 31, 2 ** 31 - 1, -10 ** 6)
    kc, vc = caches(rng, B, cap, d, [0] * B, 1e30)
    qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
    out, k2, v2 = eng.dbg_self_attention_long_ragged(qkv, kc, vc, 40, wild, cap)
    assert not out.any() and np.array_equal(bits(k2), bits(kc)) and np.array_equal(bits(v2), bits(vc))
    qkv = rng.standard_normal((4 * B, 3 * d)).astype(np.float32)
    out, k2, v2 = eng.dbg_self_attention_prefill_ragged(qkv, kc, vc, 40, 4, wild, cap)
    assert not out.any() and np.array_equal(bits(k2), bits(kc)) and np.array_equal(bits(v2), bits(vc))


def test_the_embedding_takes_the_clips_own_position(eng):
    rng = np.random.default_rng(8)
    B, K, N, V, n_pos, slot = 6, 128, 384, 50, 40, 12
    tok = rng.standard_normal((V, K)).astype(np.float32)
    pos = rng.standard_normal((n_pos, K)).astype(np.float32)
    ids = np.array([3, 49, 0, 7, 7, 12], np.int64)
    g_, b_ = (1 + 0.2 * rng.standard_normal(K)).astype(np.float32), (0.1 * rng.standard_normal(K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / 16).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    starts = np.array([0, 3, 12, 20, -27, -40], np.int32)  # positions 12, 9, 0, -8 -> 0, 39, 52 -> 39 (the clamps)
    Y, x = eng.dbg_dec_ln_gemm_ragged(W, bias, g_, b_, ids, slot, starts, tok, pos)
    for b in range(B):
        at = min(max(slot - int(starts[b]), 0), n_pos - 1)
        Y1, x1 = eng.dbg_dec_ln_gemm(W, bias, g_, b_, ids=ids[b:b + 1], pos=at, tok_emb=tok, pos_emb=pos)
        assert np.array_equal(bits(x[b]), bits(x1[0])) and np.array_equal(bits(Y[b]), bits(Y1[0])), b
        assert np.array_equal(x[b], tok[ids[b]] + pos[at])
    Y0, x0 = eng.dbg_dec_ln_gemm_ragged(W, bias, g_, b_, ids, slot, None, tok, pos)  # a null pointer: the tap as it was
    Y1, x1 = eng.dbg_dec_ln_gemm(W, bias, g_, b_, ids=ids, pos=slot, tok_emb=tok, pos_emb=pos)
    assert np.array_equal(bits(Y0), bits(Y1)) and np.array_equal(bits(x0), bits(x1))


def test_the_cap_kernel_flips_finished_at_the_last_position(eng):
    P = 78
    starts = np.array([0, 1, 5, 64, 0, 77], np.int32)
    before = np.array([0, 0, 0, 0, 1, 0], np.int32)
    for slot in (0, 76, 77, 78, 82, 141, 154):
        fin = eng.dbg_ragged_cap(slot, P, starts, before)
        want = before | (slot - starts == P - 1)
        assert np.array_equal(fin, want.astype(np.int32)), slot
