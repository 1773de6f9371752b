"""self_attention_prefill (k_attention.hip; wt_engine_set_context) through its debug tap against
float64 numpy: np new positions over a cache of up to 448 rows.  Without the feature the tap does not exist and every
test here fails."""
from ctypes import POINTER, c_float

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 1e-5  # the project's bar for this computation (test_gpu_kernels.py, standard-normal inputs)
INVALID = "WT_ERR_INVALID_ARG"
SHAPES = [(2, 1, 160), (6, 3, 448), (8, 2, 448)]  # (H, B, cap)
# (pos0, np): one position, less than a query group, groups + a remainder, the most rows a pass takes, a cache prefix that
# ends inside a key tile, either side of the old kernels' 32-row limit, late in the cache; None = cap - np
POSITIONS = [(0, 1), (0, 5), (0, 33), (0, 128), (3, 42), (31, 2), (32, 1), (60, 9), (100, 64), (320, 128),
             (None, 1), (None, 9), (None, 42), (None, 128)]


def cases():
    out = []
    for H, B, cap in SHAPES:
        for pos0, n in POSITIONS:
            p0 = cap - n if pos0 is None else pos0
            if n * B <= 128 and p0 >= 0 and p0 + n <= cap and (H, B, cap, p0, n) not in out:
                out.append((H, B, cap, p0, n))
    return out


CASES = cases()


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


_inputs = {}


def inputs(H, B, cap, pos0, n):
    """Caches with rows < pos0 standard normal and rows >= pos0 filled with 1e30, the new rows [n * B][3d] (row = p * B
    + b), and the float64 result [n * B][d]."""
    key = (H, B, cap, pos0, n)
    if key not in _inputs:
        rng = np.random.default_rng([H, B, cap, pos0, n])
        d = 64 * H
        kc = np.full((B, cap, d), 1e30, np.float32)
        vc = np.full((B, cap, d), 1e30, np.float32)
        kc[:, :pos0] = rng.standard_normal((B, pos0, d))
        vc[:, :pos0] = rng.standard_normal((B, pos0, d))
        qkv = rng.standard_normal((n * B, 3 * d)).astype(np.float32)
        new = qkv.reshape(n, B, 3, H, 64).astype(np.float64)
        ref = np.zeros((n, B, H, 64))
        causal = np.arange(pos0 + n)[None, :] <= pos0 + np.arange(n)[:, None]
        for b in range(B):
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                k = np.concatenate([kc[b, :pos0, sl].astype(np.float64), new[:, b, 1, h]])
                v = np.concatenate([vc[b, :pos0, sl].astype(np.float64), new[:, b, 2, h]])
                s = np.where(causal, (new[:, b, 0, h] @ k.T) / 8.0, -np.inf)
                p = np.exp(s - s.max(-1, keepdims=True))
                ref[:, b, h] = (p / p.sum(-1, keepdims=True)) @ v
        ref = ref.reshape(n * B, d)
        for a in (kc, vc, qkv, ref):
            a.setflags(write=False)
        _inputs[key] = (kc, vc, qkv, ref)
    return _inputs[key]


@pytest.mark.parametrize("H,B,cap,pos0,n", CASES)
def test_attends_appends_and_ignores_the_tail(eng, H, B, cap, pos0, n):
    d = 64 * H
    kc, vc, qkv, ref = inputs(H, B, cap, pos0, n)
    out, kc2, vc2 = eng.dbg_self_attention_prefill(qkv, kc, vc, pos0, n)
    err = np.abs(out - ref).max()
    print(f"H {H} B {B} cap {cap} pos0 {pos0} np {n}: max |delta| {err:.2e}")
    # rows >= pos0 hold 1e30: one of them read as a key or a value would give inf / nan or a huge output
    assert np.isfinite(out).all()
    assert err <= BAR
    # the caches after the call = the caches before it plus exactly rows pos0 .. pos0 + n - 1, bit-equal to the new k, v
    want_k, want_v = kc.copy(), vc.copy()
    new = qkv.reshape(n, B, 3, d)
    want_k[:, pos0:pos0 + n] = new[:, :, 1].transpose(1, 0, 2)
    want_v[:, pos0:pos0 + n] = new[:, :, 2].transpose(1, 0, 2)
    assert np.array_equal(kc2.view(np.uint32), want_k.view(np.uint32))
    assert np.array_equal(vc2.view(np.uint32), want_v.view(np.uint32))
    # the tail's contents do not matter: zeros instead of 1e30 from pos0 + n on give the same output bits
    kz, vz = kc.copy(), vc.copy()
    kz[:, pos0 + n:] = 0
    vz[:, pos0 + n:] = 0
    outz, _, _ = eng.dbg_self_attention_prefill(qkv, kz, vz, pos0, n)
    assert np.array_equal(outz.view(np.uint32), out.view(np.uint32))


@pytest.mark.parametrize("pos0,n", [(0, 1), (0, 33), (3, 42), (31, 2), (60, 9), (406, 42)])
def test_a_clip_is_bit_identical_alone_or_in_a_batch(eng, pos0, n):
    H, B, cap = 6, 3, 448
    d = 64 * H
    kc, vc, qkv, _ = inputs(H, B, cap, pos0, n)
    out3, _, _ = eng.dbg_self_attention_prefill(qkv, kc, vc, pos0, n)
    rows = qkv.reshape(n, B, 3 * d)
    for b in (1, 2):
        out1, _, _ = eng.dbg_self_attention_prefill(rows[:, b], kc[b:b + 1], vc[b:b + 1], pos0, n)
        assert np.array_equal(out3.reshape(n, B, d)[:, b].view(np.uint32), out1.view(np.uint32))


def test_one_launch_equals_the_same_positions_in_two(eng):
    """The order of a query's sums depends on its keys alone, not on how the positions are grouped into launches."""
    H, B, cap, pos0, n = 6, 3, 448, 3, 42
    d = 64 * H
    kc, vc, qkv, _ = inputs(H, B, cap, pos0, n)
    out, k1, v1 = eng.dbg_self_attention_prefill(qkv, kc, vc, pos0, n)
    cut = 17
    oa, ka, va = eng.dbg_self_attention_prefill(qkv[:cut * B], kc, vc, pos0, cut)
    ob, kb, vb = eng.dbg_self_attention_prefill(qkv[cut * B:], ka, va, pos0 + cut, n - cut)
    assert np.array_equal(np.concatenate([oa, ob]).view(np.uint32), out.view(np.uint32))
    assert np.array_equal(kb.view(np.uint32), k1.view(np.uint32)) and np.array_equal(vb.view(np.uint32), v1.view(np.uint32))


def test_it_agrees_with_the_one_position_kernels(eng):
    """Position by position the new kernel computes what self_attention_step and self_attention_long compute."""
    rng = np.random.default_rng(7)
    B, H, cap = 2, 2, 160
    d = 64 * H
    for pos in (0, 5, 31, 32, 100):
        kc = np.full((B, cap, d), 1e30, np.float32)
        vc = np.full((B, cap, d), 1e30, np.float32)
        kc[:, :pos] = rng.standard_normal((B, pos, d))
        vc[:, :pos] = rng.standard_normal((B, pos, d))
        qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
        a, ka, va = eng.dbg_self_attention_prefill(qkv, kc, vc, pos, 1)
        b_, kb, vb = eng.dbg_self_attention_long(qkv, kc, vc, pos)
        assert np.abs(a - b_).max() < 2 * BAR
        assert np.array_equal(ka, kb) and np.array_equal(va, vb)


def test_launcher_refusals_return_a_status(eng, pkg):
    def refused(B, H, cap, pos0, n):
        L = pkg.lib()
        Bc, Hc, capc, nc = max(B, 1), max(H, 1), max(min(cap, 448), 1), max(min(n, 128), 1)
        k = np.zeros((Bc, capc, Hc * 64), np.float32)
        v = k.copy()
        out = np.zeros((nc * Bc, Hc * 64), np.float32)
        q = np.zeros((nc * Bc, 3 * Hc * 64), np.float32)
        fp = lambda a: a.ctypes.data_as(POINTER(c_float))
        rc = L.wt_dbg_self_attention_prefill(eng.handle, B, H, cap, pos0, n, fp(q), fp(k), fp(v), fp(out))
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
    kc, vc, qkv, ref = inputs(2, 1, 160, 60, 9)
    out, _, _ = eng.dbg_self_attention_prefill(qkv, kc, vc, 60, 9)
    assert np.abs(out - ref).max() <= BAR
