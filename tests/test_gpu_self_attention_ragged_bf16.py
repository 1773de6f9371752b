"""The ragged self-attention kernels in the bf16 storage mode (option full_bf16_all) through the
taps wt_dbg_self_attention_long_ragged_bf16 and wt_dbg_self_attention_prefill_ragged_bf16: the mirror of
tests/test_gpu_self_attention_ragged.py on bf16 caches.  A clip at Whisper position slot - start[b] carries the bits of
the unragged bf16 tap at that position, output and both caches, and meets float64 numpy on the bf16-rounded operands at
the bar of sections 4.2 and 33; a clip outside [0, P) is void: zeros out, caches untouched bit for bit.  The caches
travel as float32 arrays of bf16-representable values.  Without the feature the taps do not exist and every test here
fails."""
import os
import sys
from ctypes import POINTER, c_float, c_int32

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decoder_attn_ref import bf16_round  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-5  # against float64 on the rounded operands (DESIGN sections 4.2 and 33)
INVALID = "WT_ERR_INVALID_ARG"
SLOTS = (0, 5, 31, 32, 127, 128, 129, 159, 447)  # a bf16 round trip covers 128 keys: 127 / 128 / 129 are its edges
BIG = float(bf16_round(np.full(1, 1e30, np.float32))[0])
worst = {"long": 0.0, "prefill": 0.0}


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()
    print("largest |delta| against float64 on the rounded operands: long %.2e, prefill %.2e" % (worst["long"], worst["prefill"]))


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
    """[B][cap][d] k and v of bf16 values: clip b's rows < known[b] rounded standard normal, every other row `fill`."""
    kc = np.full((B, cap, d), fill, np.float32)
    vc = np.full((B, cap, d), fill, np.float32)
    for b in range(B):
        n = max(0, min(known[b], cap))
        kc[b, :n] = bf16_round(rng.standard_normal((n, d)).astype(np.float32))
        vc[b, :n] = bf16_round(rng.standard_normal((n, d)).astype(np.float32))
    return kc, vc


@pytest.mark.parametrize("H", [2, 6])
@pytest.mark.parametrize("cap", [160, 448])
@pytest.mark.parametrize("slot", SLOTS)
def test_long_kernel_per_clip_positions(eng, H, cap, slot):
    B, d = 3, 64 * H
    for starts in ((0, 5, slot), (0, slot + 1, 0)):
        for P in sorted({cap, min(max(slot, 1), cap)}):  # at the cap, and at the slot
            q = [slot - s for s in starts]
            live = [0 <= x < P for x in q]
            rng = np.random.default_rng([H, cap, slot, P, starts[1]])
            qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
            state = rng.bit_generator.state
            kc, vc = caches(rng, B, cap, d, [x if ok else 0 for x, ok in zip(q, live)], BIG)
            out, k2, v2 = eng.dbg_self_attention_long_ragged(qkv, kc, vc, slot, starts, P, bf16=True)
            for b in range(B):
                if not live[b]:  # void: zeros, nothing appended
                    assert not out[b].any() and np.array_equal(bits(k2[b]), bits(kc[b])) and np.array_equal(bits(v2[b]), bits(vc[b]))
                    continue
                o1, k1, v1 = eng.dbg_self_attention_long(qkv[b:b + 1], kc[b:b + 1], vc[b:b + 1], q[b], bf16=True)
                assert np.array_equal(bits(out[b]), bits(o1[0])), (starts, P, b)
                assert np.array_equal(bits(k2[b]), bits(k1[0])) and np.array_equal(bits(v2[b]), bits(v1[0]))
                # the appended row is the rounded new k / v, and no other cell changed
                assert np.array_equal(bits(k2[b, q[b]]), bits(bf16_round(qkv[b, d:2 * d])))
                assert np.array_equal(bits(v2[b, q[b]]), bits(bf16_round(qkv[b, 2 * d:])))
                keep = np.arange(cap) != q[b]
                assert np.array_equal(bits(k2[b, keep]), bits(kc[b, keep])) and np.array_equal(bits(v2[b, keep]), bits(vc[b, keep]))
                keys = np.concatenate([kc[b, :q[b]], bf16_round(qkv[b:b + 1, d:2 * d])])
                vals = np.concatenate([vc[b, :q[b]], bf16_round(qkv[b:b + 1, 2 * d:])])
                err = np.abs(out[b] - attend64(qkv[b, :d], keys, vals, H)).max()
                worst["long"] = max(worst["long"], err)
                assert err <= BAR, (starts, P, b, err)
            # the stale rows and the void clips' caches do not matter: zeros in their place give the same bits
            rng.bit_generator.state = state
            kz, vz = caches(rng, B, cap, d, [x if ok else 0 for x, ok in zip(q, live)], 0.0)
            outz, _, _ = eng.dbg_self_attention_long_ragged(qkv, kz, vz, slot, starts, P, bf16=True)
            assert np.array_equal(bits(outz), bits(out))
    if slot < cap:  # all starts 0: the unragged bf16 launch, bit for bit
        rng = np.random.default_rng([H, cap, slot])
        qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
        kc, vc = caches(rng, B, cap, d, [slot] * B, BIG)
        got = eng.dbg_self_attention_long_ragged(qkv, kc, vc, slot, (0, 0, 0), cap, bf16=True)
        want = eng.dbg_self_attention_long(qkv, kc, vc, slot, bf16=True)
        assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def prefill_starts(B, pos0, n):
    """Start vectors that put a clip's position 0 before the launch's range, at its first slot, inside it, at its last
    slot and behind it — rotated over the clips."""
    choices = [0, max(pos0 - 7, 0), pos0, pos0 + 5, pos0 + 16, pos0 + n - 1, pos0 + n, pos0 + n + 9]
    return [tuple(choices[(i + b) % len(choices)] for b in range(B)) for i in range(len(choices))]


PREFILL = [(3, 0, 16), (3, 5, 20), (3, 120, 17), (5, 224, 4)]  # (B, pos0, np)


@pytest.mark.parametrize("B,pos0,n", PREFILL)
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
            kc, vc = caches(rng, B, cap, d, known, BIG)
            out, k2, v2 = eng.dbg_self_attention_prefill_ragged(qkv, kc, vc, pos0, n, starts, P, bf16=True)
            out = out.reshape(n, B, d)
            for b in range(B):
                if lo[b] >= hi[b]:  # the whole clip is void: zeros, nothing appended
                    assert not out[:, b].any() and np.array_equal(bits(k2[b]), bits(kc[b])) and np.array_equal(bits(v2[b]), bits(vc[b]))
                    continue
                assert not out[:lo[b], b].any() and not out[hi[b]:, b].any()  # void queries next to live ones
                first = q0[b] + lo[b]
                o1, k1, v1 = eng.dbg_self_attention_prefill(np.ascontiguousarray(rows[lo[b]:hi[b], b]), kc[b:b + 1], vc[b:b + 1],
                                                            first, hi[b] - lo[b], bf16=True)
                assert np.array_equal(bits(out[lo[b]:hi[b], b]), bits(o1)), (starts, P, b)
                assert np.array_equal(bits(k2[b]), bits(k1[0])) and np.array_equal(bits(v2[b]), bits(v1[0]))
                # the live queries' rows appended rounded, every other cell as it was
                last = first + hi[b] - lo[b]
                assert np.array_equal(bits(k2[b, first:last]), bits(bf16_round(rows[lo[b]:hi[b], b, d:2 * d])))
                assert np.array_equal(bits(v2[b, first:last]), bits(bf16_round(rows[lo[b]:hi[b], b, 2 * d:])))
                assert np.array_equal(bits(k2[b, :first]), bits(kc[b, :first])) and np.array_equal(bits(k2[b, last:]), bits(kc[b, last:]))
                assert np.array_equal(bits(v2[b, :first]), bits(vc[b, :first])) and np.array_equal(bits(v2[b, last:]), bits(vc[b, last:]))
                keys = np.concatenate([kc[b, :first], bf16_round(rows[lo[b]:hi[b], b, d:2 * d])])
                vals = np.concatenate([vc[b, :first], bf16_round(rows[lo[b]:hi[b], b, 2 * d:])])
                for p in (lo[b], (lo[b] + hi[b]) // 2, hi[b] - 1):  # the first, a middle and the last live query
                    nk = q0[b] + p + 1
                    err = np.abs(out[p, b] - attend64(rows[p, b, :d], keys[:nk], vals[:nk], H)).max()
                    worst["prefill"] = max(worst["prefill"], err)
                    assert err <= BAR, (starts, P, b, p, err)
            rng.bit_generator.state = state
            kz, vz = caches(rng, B, cap, d, known, 0.0)
            outz, _, _ = eng.dbg_self_attention_prefill_ragged(qkv, kz, vz, pos0, n, starts, P, bf16=True)
            assert np.array_equal(bits(outz.reshape(n, B, d)), bits(out))
    # all starts 0: the unragged bf16 launch, bit for bit
    rng = np.random.default_rng([B, pos0, n])
    qkv = rng.standard_normal((n * B, 3 * d)).astype(np.float32)
    kc, vc = caches(rng, B, cap, d, [pos0] * B, BIG)
    got = eng.dbg_self_attention_prefill_ragged(qkv, kc, vc, pos0, n, (0,) * B, cap, bf16=True)
    want = eng.dbg_self_attention_prefill(qkv, kc, vc, pos0, n, bf16=True)
    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


@pytest.mark.parametrize("B,pos0,n", PREFILL)
def test_prefill_one_launch_equals_two(eng, B, pos0, n):
    """Keys taken from qkv are rounded as the appended rows are: np positions in one launch or in two, at three cuts."""
    H, cap = 6, 448
    d = 64 * H
    starts = tuple([0, 3, pos0 + 2, 1, pos0 + n][b % 5] for b in range(B))  # live throughout, from inside, void
    rng = np.random.default_rng([B, pos0, n, 77])
    qkv = rng.standard_normal((n * B, 3 * d)).astype(np.float32)
    kc, vc = caches(rng, B, cap, d, [max(pos0 - s, 0) for s in starts], BIG)
    one = eng.dbg_self_attention_prefill_ragged(qkv, kc, vc, pos0, n, starts, cap, bf16=True)
    for cut in sorted({1, n // 2, n - 1}):
        o1, k1, v1 = eng.dbg_self_attention_prefill_ragged(qkv[:cut * B], kc, vc, pos0, cut, starts, cap, bf16=True)
        o2, k2, v2 = eng.dbg_self_attention_prefill_ragged(qkv[cut * B:], k1, v1, pos0 + cut, n - cut, starts, cap, bf16=True)
        assert np.array_equal(bits(np.concatenate([o1, o2])), bits(one[0])), cut
        assert np.array_equal(bits(k2), bits(one[1])) and np.array_equal(bits(v2), bits(one[2])), cut


def test_the_launchers_refuse_what_the_fp32_ragged_forms_refuse(eng, pkg):
    """Every refusal of the fp32 ragged launchers, with the output untouched, and the next launch right."""
    L = pkg.lib()
    fp = lambda a: a.ctypes.data_as(POINTER(c_float))  # noqa: E731

    def arrays(B, H, cap, n):
        Bc, Hc, capc, nc = max(B, 1), max(H, 1), max(min(cap, 448), 1), max(min(n, 128), 1)
        k = np.full((Bc, capc, Hc * 64), 3.0, np.float32)
        return (np.zeros((nc * Bc, 3 * Hc * 64), np.float32), k, k.copy(), np.full((nc * Bc, Hc * 64), 7.0, np.float32),
                np.zeros(Bc, np.int32))

    def untouched(k, v, o):
        return bool((k == 3.0).all() and (v == 3.0).all() and (o == 7.0).all())

    def long_(B, H, cap, pos, P, start=True, bf=True):
        q, k, v, o, s = arrays(B, H, cap, 1)
        sp = s.ctypes.data_as(POINTER(c_int32)) if start else None
        fn = L.wt_dbg_self_attention_long_ragged_bf16 if bf else L.wt_dbg_self_attention_long_ragged
        st = pkg.STATUS_NAMES.get(fn(eng.handle, B, H, cap, pos, fp(q), fp(k), fp(v), fp(o), sp, P))
        return st, untouched(k, v, o)

    def prefill(B, H, cap, pos0, n, P, start=True, bf=True):
        q, k, v, o, s = arrays(B, H, cap, n)
        sp = s.ctypes.data_as(POINTER(c_int32)) if start else None
        fn = L.wt_dbg_self_attention_prefill_ragged_bf16 if bf else L.wt_dbg_self_attention_prefill_ragged
        st = pkg.STATUS_NAMES.get(fn(eng.handle, B, H, cap, pos0, n, fp(q), fp(k), fp(v), fp(o), sp, P))
        return st, untouched(k, v, o)

    long_cases = [(3, 2, 160, -1, 160), (3, 2, 449, 10, 449), (0, 2, 160, 10, 160), (3, 0, 160, 10, 160), (3, 2, 160, 10, 0),
                  (3, 2, 160, 10, 161), (3, 2, 160, 896, 160), (3, 2, 160, 200, 160), (3, 2, 160, 10, 160)]
    for case in long_cases:
        want = long_(*case, bf=False)[0]
        got, same = long_(*case)
        assert got == want and (same or got == "WT_OK"), case  # refused: nothing was written
    assert [long_(*c, bf=False)[0] for c in long_cases] == [INVALID] * 7 + ["WT_OK"] * 2
    assert long_(3, 2, 160, 10, 160, start=False) == (INVALID, True)
    prefill_cases = [(3, 2, 160, -1, 4, 160), (3, 2, 160, 10, 0, 160), (3, 2, 160, 157, 4, 160), (3, 2, 449, 10, 4, 449),
                     (3, 2, 448, 10, 43, 448), (0, 2, 160, 40, 4, 160), (3, 0, 160, 40, 4, 160), (3, 2, 160, 40, 4, 0),
                     (3, 2, 160, 40, 4, 161), (3, 2, 448, 406, 42, 448)]
    for case in prefill_cases:
        want = prefill(*case, bf=False)[0]
        got, same = prefill(*case)
        assert got == want and (same or got == "WT_OK"), case
    assert [prefill(*c, bf=False)[0] for c in prefill_cases] == [INVALID] * 9 + ["WT_OK"]
    assert prefill(3, 2, 160, 40, 4, 160, start=False) == (INVALID, True)
    # and the launch behind the refusals is right
    H, B, cap, slot = 2, 3, 160, 40
    d = 64 * H
    rng = np.random.default_rng(3)
    qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
    kc, vc = caches(rng, B, cap, d, [slot] * B, BIG)
    got = eng.dbg_self_attention_long_ragged(qkv, kc, vc, slot, (0, 0, 0), cap, bf16=True)
    want = eng.dbg_self_attention_long(qkv, kc, vc, slot, bf16=True)
    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def test_a_wild_start_array_touches_nothing(eng):
    """Every index derived from the start array is bounded inside the kernels: starts far outside any chain make void
    clips, whatever they hold."""
    H, B, cap = 2, 3, 160
    d = 64 * H
    rng = np.random.default_rng(11)
    wild = (-2 ** 31, 2 ** 31 - 1, -10 ** 6)
    kc, vc = caches(rng, B, cap, d, [0] * B, BIG)
    qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
    out, k2, v2 = eng.dbg_self_attention_long_ragged(qkv, kc, vc, 40, wild, cap, bf16=True)
    assert not out.any() and np.array_equal(bits(k2), bits(kc)) and np.array_equal(bits(v2), bits(vc))
    qkv = rng.standard_normal((4 * B, 3 * d)).astype(np.float32)
    out, k2, v2 = eng.dbg_self_attention_prefill_ragged(qkv, kc, vc, 40, 4, wild, cap, bf16=True)
    assert not out.any() and np.array_equal(bits(k2), bits(kc)) and np.array_equal(bits(v2), bits(vc))
