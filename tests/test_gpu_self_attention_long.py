"""self_attention_long (k_attention.hip; option max_positions) through its debug tap against
float64 numpy: one new position over a cache of up to 448 rows.  Without the feature the tap does not exist and every
test here fails."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 1e-5  # the project's bar for this computation (test_gpu_kernels.py, standard-normal inputs)
INVALID = "WT_ERR_INVALID_ARG"
# (cap, pos): the first new position, the boundaries of a 64-key round and of the 16-lane groups' last partial round,
# the last row of either cache size
CASES = [(160, 32), (160, 33), (160, 63), (160, 64), (160, 65), (160, 127), (160, 128), (160, 159), (448, 447)]


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


_inputs = {}


def inputs(B, H, cap, pos):
    """Caches with rows < pos standard normal and rows >= pos filled with 1e30, the new rows, and the float64 result."""
    key = (B, H, cap, pos)
    if key not in _inputs:
        rng = np.random.default_rng(cap * 1000 + pos * 10 + H)
        d = 64 * H
        kc = np.full((B, cap, d), 1e30, np.float32)
        vc = np.full((B, cap, d), 1e30, np.float32)
        kc[:, :pos] = rng.standard_normal((B, pos, d))
        vc[:, :pos] = rng.standard_normal((B, pos, d))
        qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
        ref = np.zeros((B, d))
        for b in range(B):
            k = np.concatenate([kc[b, :pos], qkv[b:b + 1, d:2 * d]]).astype(np.float64)
            v = np.concatenate([vc[b, :pos], qkv[b:b + 1, 2 * d:]]).astype(np.float64)
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                ref[b, sl] = attn_ref(qkv[b:b + 1, sl].astype(np.float64), k[:, sl], v[:, sl])[0]
        for a in (kc, vc, qkv, ref):
            a.setflags(write=False)
        _inputs[key] = (kc, vc, qkv, ref)
    return _inputs[key]


@pytest.mark.parametrize("H", [2, 6])
@pytest.mark.parametrize("cap,pos", CASES)
def test_attends_appends_and_ignores_the_tail(eng, H, cap, pos):
    B, d = 3, 64 * H
    kc, vc, qkv, ref = inputs(B, H, cap, pos)
    out, kc2, vc2 = eng.dbg_self_attention_long(qkv, kc, vc, pos)
    err = np.abs(out - ref).max()
    print(f"H {H} cap {cap} pos {pos}: max |delta| {err:.2e}")
    # rows > pos hold 1e30: one of them read as a key or a value would give inf / nan or a huge output
    assert np.isfinite(out).all()
    assert err < BAR
    # the cache after the call = the cache before it plus exactly row pos
    want_k, want_v = kc.copy(), vc.copy()
    want_k[:, pos] = qkv[:, d:2 * d]
    want_v[:, pos] = qkv[:, 2 * d:]
    assert np.array_equal(kc2, want_k) and np.array_equal(vc2, want_v)


@pytest.mark.parametrize("cap,pos", [(160, 32), (160, 65), (160, 159), (448, 447)])
def test_a_row_is_bit_identical_alone_or_in_a_batch(eng, cap, pos):
    H, d = 6, 384
    kc, vc, qkv, _ = inputs(3, H, cap, pos)
    out3, _, _ = eng.dbg_self_attention_long(qkv, kc, vc, pos)
    out1, _, _ = eng.dbg_self_attention_long(qkv[1:2], kc[1:2], vc[1:2], pos)
    assert np.array_equal(out3[1], out1[0])
    # and the tail's contents do not matter: zeros instead of 1e30 past pos give the same bits
    kz, vz = kc.copy(), vc.copy()
    kz[:, pos:] = 0
    vz[:, pos:] = 0
    outz, _, _ = eng.dbg_self_attention_long(qkv, kz, vz, pos)
    assert np.array_equal(outz, out3)


def test_the_old_kernel_still_serves_position_31(eng, pkg):
    """The launcher split did not move self_attention_step: pos 31 of a 32-row cache through the existing tap."""
    rng = np.random.default_rng(31)
    B, H, cap, pos = 3, 2, 32, 31
    d = 64 * H
    kc = np.zeros((B, cap, d), np.float32)
    vc = np.zeros((B, cap, d), np.float32)
    kc[:, :pos] = rng.standard_normal((B, pos, d))
    vc[:, :pos] = rng.standard_normal((B, pos, d))
    qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
    out, kc2, vc2 = eng.dbg_self_attention(qkv, kc, vc, pos)
    kc[:, pos] = qkv[:, d:2 * d]
    vc[:, pos] = qkv[:, 2 * d:]
    assert np.array_equal(kc2, kc) and np.array_equal(vc2, vc)
    for b in range(B):
        for h in range(H):
            sl = slice(h * 64, (h + 1) * 64)
            ref = attn_ref(qkv[b:b + 1, sl].astype(np.float64), kc[b, :, sl].astype(np.float64), vc[b, :, sl].astype(np.float64))
            assert np.abs(out[b, sl] - ref[0]).max() < BAR
    # ... and it goes on refusing what lies past its 32 rows
    with pytest.raises(pkg.WtError) as e:
        eng.dbg_self_attention(qkv, np.zeros((B, 64, d), np.float32), np.zeros((B, 64, d), np.float32), 32)
    assert str(e.value).split(":")[0] == INVALID


def test_the_long_kernel_agrees_with_the_old_one_below_32(eng):
    """Any position in [0, cap) is inside the new kernel's contract (the engine uses it from 32 on): positions 0, 5 and 31."""
    rng = np.random.default_rng(5)
    B, H, cap = 2, 2, 160
    d = 64 * H
    for pos in (0, 5, 31):
        kc = np.full((B, cap, d), 1e30, np.float32)
        vc = np.full((B, cap, d), 1e30, np.float32)
        kc[:, :pos] = rng.standard_normal((B, pos, d))
        vc[:, :pos] = rng.standard_normal((B, pos, d))
        qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
        a, ka, va = eng.dbg_self_attention_long(qkv, kc, vc, pos)
        b_, kb, vb = eng.dbg_self_attention(qkv, kc[:, :32], vc[:, :32], pos)
        assert np.abs(a - b_).max() < 2 * BAR
        assert np.array_equal(ka[:, :32], kb) and np.array_equal(va[:, :32], vb)


def test_launcher_refusals_return_a_status(eng, pkg):
    def refused(B, H, cap, pos):
        L = pkg.lib()
        k = np.zeros((max(B, 1), max(min(cap, 448), 1), max(H, 1) * 64), np.float32)
        v = k.copy()
        out = np.zeros((max(B, 1), max(H, 1) * 64), np.float32)
        q = np.zeros((max(B, 1), 3 * max(H, 1) * 64), np.float32)
        from ctypes import POINTER, c_float
        fp = lambda a: a.ctypes.data_as(POINTER(c_float))
        rc = L.wt_dbg_self_attention_long(eng.handle, B, H, cap, pos, fp(q), fp(k), fp(v), fp(out))
        return pkg.STATUS_NAMES.get(rc)

    assert refused(3, 2, 160, -1) == INVALID
    assert refused(3, 2, 160, 160) == INVALID
    assert refused(3, 2, 449, 10) == INVALID
    assert refused(0, 2, 160, 40) == INVALID
    assert refused(3, 0, 160, 40) == INVALID
    assert refused(3, 2, 448, 447) == "WT_OK"
    # the engine is unharmed
    kc, vc, qkv, ref = inputs(3, 2, 160, 64)
    out, _, _ = eng.dbg_self_attention_long(qkv, kc, vc, 64)
    assert np.abs(out - ref).max() < BAR
