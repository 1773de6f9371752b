"""self_attention_long<false, false, true> (k_attention.hip; option full_bf16) through its debug
tap against float64 numpy on the bf16-rounded operands: one new position over a bf16 cache of up to 448 rows.  The
cases are those of test_gpu_self_attention_long.py.  Without the feature the tap does not exist and every test here
fails."""
import os
import sys
from ctypes import POINTER, c_float

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decoder_attn_ref import bf16_round  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-5  # the project's bar for this computation, which DESIGN section 4.2 holds self_attention_step<true> to
INVALID = "WT_ERR_INVALID_ARG"
CASES = [(160, 32), (160, 33), (160, 63), (160, 64), (160, 65), (160, 127), (160, 128), (160, 159), (448, 447)]
HUGE = bf16_round(np.float32(1e30))[()]


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def attn_ref(q, k, v):
    s = (q @ k.T) / 8.0
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    return (p / p.sum(-1, keepdims=True)) @ v


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_inputs = {}


def inputs(B, H, cap, pos):
    """bf16-representable caches with rows < pos standard normal and rows >= pos filled with bf16(1e30), the new rows
    (fp32: q stays as it is, the kernel rounds k and v), and the float64 result on the rounded k and v."""
    key = (B, H, cap, pos)
    if key not in _inputs:
        rng = np.random.default_rng(cap * 1000 + pos * 10 + H + 33)
        d = 64 * H
        kc = np.full((B, cap, d), HUGE, np.float32)
        vc = np.full((B, cap, d), HUGE, np.float32)
        kc[:, :pos] = bf16_round(rng.standard_normal((B, pos, d)))
        vc[:, :pos] = bf16_round(rng.standard_normal((B, pos, d)))
        qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
        knew, vnew = bf16_round(qkv[:, d:2 * d]), bf16_round(qkv[:, 2 * d:])
        ref = np.zeros((B, d))
        for b in range(B):
            k = np.concatenate([kc[b, :pos], knew[b:b + 1]]).astype(np.float64)
            v = np.concatenate([vc[b, :pos], vnew[b:b + 1]]).astype(np.float64)
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                ref[b, sl] = attn_ref(qkv[b:b + 1, sl].astype(np.float64), k[:, sl], v[:, sl])[0]
        for a in (kc, vc, qkv, ref):
            a.setflags(write=False)
        _inputs[key] = (kc, vc, qkv, ref)
    return _inputs[key]


@pytest.mark.parametrize("H", [2, 6])
@pytest.mark.parametrize("cap,pos", CASES)
def test_attends_appends_the_roundings_and_ignores_the_tail(eng, H, cap, pos):
    B, d = 3, 64 * H
    kc, vc, qkv, ref = inputs(B, H, cap, pos)
    out, kc2, vc2 = eng.dbg_self_attention_long(qkv, kc, vc, pos, bf16=True)
    err = np.abs(out - ref).max()
    print(f"H {H} cap {cap} pos {pos}: max |delta| {err:.2e}")
    # rows > pos hold 1e30: one of them read as a key or a value would give inf / nan or a huge output
    assert np.isfinite(out).all()
    assert err < BAR
    # the cache after the call = the cache before it plus exactly row pos, and that row is the rounding, bit for bit
    want_k, want_v = kc.copy(), vc.copy()
    want_k[:, pos] = bf16_round(qkv[:, d:2 * d])
    want_v[:, pos] = bf16_round(qkv[:, 2 * d:])
    assert np.array_equal(bits(kc2), bits(want_k)) and np.array_equal(bits(vc2), bits(want_v))


@pytest.mark.parametrize("cap,pos", [(160, 32), (160, 65), (160, 159), (448, 447)])
def test_a_row_is_bit_identical_alone_or_in_a_batch(eng, cap, pos):
    H = 6
    kc, vc, qkv, _ = inputs(3, H, cap, pos)
    out3, _, _ = eng.dbg_self_attention_long(qkv, kc, vc, pos, bf16=True)
    out1, _, _ = eng.dbg_self_attention_long(qkv[1:2], kc[1:2], vc[1:2], pos, bf16=True)
    assert np.array_equal(bits(out3[1]), bits(out1[0]))
    # and the tail's contents do not matter: zeros instead of 1e30 past pos give the same bits
    kz, vz = kc.copy(), vc.copy()
    kz[:, pos:] = 0
    vz[:, pos:] = 0
    outz, _, _ = eng.dbg_self_attention_long(qkv, kz, vz, pos, bf16=True)
    assert np.array_equal(bits(outz), bits(out3))


def test_it_takes_over_the_cache_of_the_step_kernel(eng):
    """Rows 0 .. 31 written by self_attention_step<true>, position by position, then read at pos = 32: the two kernels
    share one cache layout and one rounding."""
    rng = np.random.default_rng(3233)
    B, H, cap = 3, 2, 160
    d = 64 * H
    kc = np.full((B, cap, d), HUGE, np.float32)
    vc = np.full((B, cap, d), HUGE, np.float32)
    rows = rng.standard_normal((33, B, 3 * d)).astype(np.float32)
    for pos0 in range(0, 32, 4):  # (the step kernel's tap takes caches of at most 32 staged rows: four positions a call)
        _, k32, v32 = eng.dbg_self_attention(rows[pos0:pos0 + 4].reshape(4 * B, 3 * d), kc[:, :32], vc[:, :32], pos0, 4, bf16=True)
        kc[:, :32], vc[:, :32] = k32, v32
    want_k = bf16_round(rows[:32, :, d:2 * d]).transpose(1, 0, 2)
    want_v = bf16_round(rows[:32, :, 2 * d:]).transpose(1, 0, 2)
    assert np.array_equal(bits(kc[:, :32]), bits(want_k)) and np.array_equal(bits(vc[:, :32]), bits(want_v))
    out, kc2, vc2 = eng.dbg_self_attention_long(rows[32], kc, vc, 32, bf16=True)
    assert np.array_equal(bits(kc2[:, :32]), bits(want_k)) and np.array_equal(bits(vc2[:, :32]), bits(want_v))
    k = np.concatenate([want_k, bf16_round(rows[32, :, None, d:2 * d])], axis=1).astype(np.float64)
    v = np.concatenate([want_v, bf16_round(rows[32, :, None, 2 * d:])], axis=1).astype(np.float64)
    for b in range(B):
        for h in range(H):
            sl = slice(h * 64, (h + 1) * 64)
            ref = attn_ref(rows[32, b:b + 1, sl].astype(np.float64), k[b][:, sl], v[b][:, sl])[0]
            assert np.abs(out[b, sl] - ref).max() < BAR


def test_launcher_refusals_return_a_status(eng, pkg):
    def refused(B, H, cap, pos):
        L = pkg.lib()
        k = np.zeros((max(B, 1), max(min(cap, 448), 1), max(H, 1) * 64), np.float32)
        v = k.copy()
        out = np.zeros((max(B, 1), max(H, 1) * 64), np.float32)
        q = np.zeros((max(B, 1), 3 * max(H, 1) * 64), np.float32)
        fp = lambda a: a.ctypes.data_as(POINTER(c_float))
        rc = L.wt_dbg_self_attention_long_bf16(eng.handle, B, H, cap, pos, fp(q), fp(k), fp(v), fp(out))
        return pkg.STATUS_NAMES.get(rc)

    assert refused(3, 2, 160, -1) == INVALID
    assert refused(3, 2, 160, 160) == INVALID
    assert refused(3, 2, 449, 10) == INVALID
    assert refused(0, 2, 160, 40) == INVALID
    assert refused(3, 0, 160, 40) == INVALID
    assert refused(3, 2, 448, 447) == "WT_OK"
    # the engine is unharmed
    kc, vc, qkv, ref = inputs(3, 2, 160, 64)
    out, _, _ = eng.dbg_self_attention_long(qkv, kc, vc, 64, bf16=True)
    assert np.abs(out - ref).max() < BAR
