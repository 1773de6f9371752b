"""self_attention_prefill<false, true> (k_attention.hip; option full_bf16) through its debug tap
against float64 numpy on the bf16-rounded operands: np new positions over a bf16 cache of up to 448 rows.  Every key row
taken from qkv is rounded as the appended rows are, so one launch equals the same positions in two.  Without the
feature the tap does not exist and every test here fails."""
import os
import sys
from ctypes import POINTER, c_float

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decoder_attn_ref import bf16_round  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-5  # the project's bar for this computation (test_gpu_self_attention_long_bf16.py)
INVALID = "WT_ERR_INVALID_ARG"
HUGE = bf16_round(np.float32(1e30))[()]
H, CAP = 6, 448
# (B, pos0, np): the most rows a pass takes from an empty cache, a cache prefix of whole key tiles, several clips with a
# short prompt, many clips late in the cache, the last rows of the cache
CASES = [(1, 0, 128), (1, 128, 100), (5, 0, 25), (32, 224, 4), (2, 440, 8)]


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_inputs = {}


def inputs(B, pos0, n):
    """bf16-representable caches with rows < pos0 standard normal and rows >= pos0 filled with bf16(1e30), the new rows
    [n * B][3d] (row = p * B + b, fp32), and the float64 result [n * B][d] on the rounded k and v."""
    key = (B, pos0, n)
    if key not in _inputs:
        rng = np.random.default_rng([33, B, pos0, n])
        d = 64 * H
        kc = np.full((B, CAP, d), HUGE, np.float32)
        vc = np.full((B, CAP, d), HUGE, np.float32)
        kc[:, :pos0] = bf16_round(rng.standard_normal((B, pos0, d)).astype(np.float32))
        vc[:, :pos0] = bf16_round(rng.standard_normal((B, pos0, d)).astype(np.float32))
        qkv = rng.standard_normal((n * B, 3 * d)).astype(np.float32)
        new = qkv.reshape(n, B, 3, H, 64)
        q = new[:, :, 0].astype(np.float64)
        knew = bf16_round(new[:, :, 1]).astype(np.float64)
        vnew = bf16_round(new[:, :, 2]).astype(np.float64)
        ref = np.zeros((n, B, H, 64))
        causal = np.arange(pos0 + n)[None, :] <= pos0 + np.arange(n)[:, None]
        for b in range(B):
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                k = np.concatenate([kc[b, :pos0, sl].astype(np.float64), knew[:, b, h]])
                v = np.concatenate([vc[b, :pos0, sl].astype(np.float64), vnew[:, b, h]])
                s = np.where(causal, (q[:, b, h] @ k.T) / 8.0, -np.inf)
                p = np.exp(s - s.max(-1, keepdims=True))
                ref[:, b, h] = (p / p.sum(-1, keepdims=True)) @ v
        ref = ref.reshape(n * B, d)
        for a in (kc, vc, qkv, ref):
            a.setflags(write=False)
        _inputs[key] = (kc, vc, qkv, ref)
    return _inputs[key]


@pytest.mark.parametrize("B,pos0,n", CASES)
def test_attends_appends_the_roundings_and_ignores_the_tail(eng, B, pos0, n):
    d = 64 * H
    kc, vc, qkv, ref = inputs(B, pos0, n)
    out, kc2, vc2 = eng.dbg_self_attention_prefill(qkv, kc, vc, pos0, n, bf16=True)
    err = np.abs(out - ref).max()
    print(f"B {B} pos0 {pos0} np {n}: max |delta| {err:.2e}")
    # rows >= pos0 hold 1e30: one of them read as a key or a value would give inf / nan or a huge output
    assert np.isfinite(out).all()
    assert err < BAR
    # the caches after the call = the caches before it plus exactly rows pos0 .. pos0 + n - 1: the roundings, bit for bit
    want_k, want_v = kc.copy(), vc.copy()
    new = qkv.reshape(n, B, 3, d)
    want_k[:, pos0:pos0 + n] = bf16_round(new[:, :, 1]).transpose(1, 0, 2)
    want_v[:, pos0:pos0 + n] = bf16_round(new[:, :, 2]).transpose(1, 0, 2)
    assert np.array_equal(bits(kc2), bits(want_k)) and np.array_equal(bits(vc2), bits(want_v))
    # nothing at or past pos0 + np is read: zeros instead of 1e30 there give the same output bits
    kz, vz = kc.copy(), vc.copy()
    kz[:, pos0 + n:] = 0
    vz[:, pos0 + n:] = 0
    outz, _, _ = eng.dbg_self_attention_prefill(qkv, kz, vz, pos0, n, bf16=True)
    assert np.array_equal(bits(outz), bits(out))


@pytest.mark.parametrize("B,pos0,n,cut", [(1, 0, 128, 50), (1, 128, 100, 17), (5, 0, 25, 16), (32, 224, 4, 1), (2, 440, 8, 3)])
def test_one_launch_equals_the_same_positions_in_two(eng, B, pos0, n, cut):
    """A key contributes the same values whether it came from qkv (rounded on the way) or was read back from the cache."""
    kc, vc, qkv, _ = inputs(B, pos0, n)
    out, k1, v1 = eng.dbg_self_attention_prefill(qkv, kc, vc, pos0, n, bf16=True)
    oa, ka, va = eng.dbg_self_attention_prefill(qkv[:cut * B], kc, vc, pos0, cut, bf16=True)
    ob, kb, vb = eng.dbg_self_attention_prefill(qkv[cut * B:], ka, va, pos0 + cut, n - cut, bf16=True)
    assert np.array_equal(bits(np.concatenate([oa, ob])), bits(out))
    assert np.array_equal(bits(kb), bits(k1)) and np.array_equal(bits(vb), bits(v1))


@pytest.mark.parametrize("B,pos0,n", [(5, 0, 25), (32, 224, 4), (2, 440, 8)])
def test_a_clip_is_bit_identical_alone_or_in_a_batch(eng, B, pos0, n):
    d = 64 * H
    kc, vc, qkv, _ = inputs(B, pos0, n)
    outb, _, _ = eng.dbg_self_attention_prefill(qkv, kc, vc, pos0, n, bf16=True)
    rows = qkv.reshape(n, B, 3 * d)
    for b in (0, B - 1):
        out1, _, _ = eng.dbg_self_attention_prefill(rows[:, b], kc[b:b + 1], vc[b:b + 1], pos0, n, bf16=True)
        assert np.array_equal(bits(outb.reshape(n, B, d)[:, b]), bits(out1))


def test_it_hands_over_to_the_long_kernel(eng):
    """A prompt appended by the prefill kernel, then one position by self_attention_long<.., true>: the same bits as the
    prefill kernel gives for that position."""
    B, pos0, n = 2, 440, 8
    d = 64 * H
    kc, vc, qkv, _ = inputs(B, pos0, n)
    out, k1, v1 = eng.dbg_self_attention_prefill(qkv, kc, vc, pos0, n, bf16=True)
    _, ka, va = eng.dbg_self_attention_prefill(qkv[:(n - 1) * B], kc, vc, pos0, n - 1, bf16=True)
    ol, kl, vl = eng.dbg_self_attention_long(qkv[(n - 1) * B:], ka, va, pos0 + n - 1, bf16=True)
    assert np.array_equal(bits(kl), bits(k1)) and np.array_equal(bits(vl), bits(v1))
    assert np.abs(ol - out[(n - 1) * B:]).max() < 2 * BAR


def test_launcher_refusals_return_a_status(eng, pkg):
    def refused(B, Hh, cap, pos0, n):
        L = pkg.lib()
        Bc, Hc, capc, nc = max(B, 1), max(Hh, 1), max(min(cap, 448), 1), max(min(n, 128), 1)
        k = np.zeros((Bc, capc, Hc * 64), np.float32)
        v = k.copy()
        out = np.zeros((nc * Bc, Hc * 64), np.float32)
        q = np.zeros((nc * Bc, 3 * Hc * 64), np.float32)
        fp = lambda a: a.ctypes.data_as(POINTER(c_float))
        rc = L.wt_dbg_self_attention_prefill_bf16(eng.handle, B, Hh, cap, pos0, n, fp(q), fp(k), fp(v), fp(out))
        return pkg.STATUS_NAMES.get(rc)

    assert refused(3, 2, 160, -1, 4) == INVALID
    assert refused(3, 2, 160, 10, 0) == INVALID
    assert refused(3, 2, 160, 10, -3) == INVALID
    assert refused(3, 2, 160, 157, 4) == INVALID   # pos0 + np > cap
    assert refused(3, 2, 160, 160, 1) == INVALID
    assert refused(3, 2, 449, 10, 4) == INVALID
    assert refused(3, 2, 448, 10, 43) == INVALID   # 129 rows
    assert refused(1, 2, 448, 10, 129) == INVALID
    assert refused(0, 2, 160, 40, 4) == INVALID
    assert refused(3, 0, 160, 40, 4) == INVALID
    assert refused(3, 2, 160, 40, 2 ** 31 - 1) == INVALID
    assert refused(3, 2, 448, 406, 42) == "WT_OK"
    # the engine is unharmed
    kc, vc, qkv, ref = inputs(2, 440, 8)
    out, _, _ = eng.dbg_self_attention_prefill(qkv, kc, vc, 440, 8, bf16=True)
    assert np.abs(out - ref).max() < BAR
