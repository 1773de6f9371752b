"""The gathered bf16 form self_attention_long<false, true, true> (k_attention.hip; option full_bf16, DESIGN.md section
33) through its debug tap against float64 numpy on the bf16-rounded operands: up to 128 rows share one bf16 cache, and
row r reads key k < pos from cache row min(anc[r][k], rows - 1).  Without the feature the tap does not exist and every
test here fails."""
import os
import sys
from ctypes import POINTER, c_float, c_uint8

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decoder_attn_ref import bf16_round  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-5  # the project's bar for this computation (test_gpu_self_attention_long_bf16.py)
INVALID = "WT_ERR_INVALID_ARG"
HUGE = bf16_round(np.float32(1e30))[()]
# (rows, H, cap, pos): one row, a few, the beam chain's 125 and the most a pass takes, at the first position behind the
# step kernel, behind a 64-key boundary and at the last row of the long cache
CASES = [(R, H, 448 if pos == 447 else 160, pos) for R, H in ((1, 2), (5, 6), (125, 6), (128, 2)) for pos in (32, 65, 447)]


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


def gathered(cache, anc, r, pos):
    """Row r's keys 0 .. pos - 1 as the kernel must read them: [pos][d]."""
    rows = cache.shape[0]
    src = np.minimum(anc[r, :pos].astype(np.int64), rows - 1)
    return cache[src, np.arange(pos)]


_inputs = {}


def inputs(R, H, cap, pos):
    """bf16-representable caches with positions < pos standard normal and positions >= pos filled with bf16(1e30), the
    new rows, a random table (entries at k >= pos hold 255: they must not be read) and the float64 result."""
    key = (R, H, cap, pos)
    if key not in _inputs:
        rng = np.random.default_rng(cap * 1000 + pos * 10 + H + 7 * R + 33)
        d = 64 * H
        kc = np.full((R, cap, d), HUGE, np.float32)
        vc = np.full((R, cap, d), HUGE, np.float32)
        kc[:, :pos] = bf16_round(rng.standard_normal((R, pos, d)).astype(np.float32))
        vc[:, :pos] = bf16_round(rng.standard_normal((R, pos, d)).astype(np.float32))
        qkv = rng.standard_normal((R, 3 * d)).astype(np.float32)
        knew, vnew = bf16_round(qkv[:, d:2 * d]), bf16_round(qkv[:, 2 * d:])
        anc = np.full((R, cap), 255, np.uint8)
        anc[:, :pos] = rng.integers(0, R, size=(R, pos))
        ref = np.zeros((R, d))
        for r in range(R):
            k = np.concatenate([gathered(kc, anc, r, pos), knew[r:r + 1]]).astype(np.float64).reshape(pos + 1, H, 64)
            v = np.concatenate([gathered(vc, anc, r, pos), vnew[r:r + 1]]).astype(np.float64).reshape(pos + 1, H, 64)
            q = qkv[r, :d].astype(np.float64).reshape(H, 64)
            s = np.einsum("hc,nhc->hn", q, k) / 8.0
            w = np.exp(s - s.max(-1, keepdims=True))
            w /= w.sum(-1, keepdims=True)
            ref[r] = np.einsum("hn,nhc->hc", w, v).reshape(d)
        for a in (kc, vc, qkv, anc, ref):
            a.setflags(write=False)
        _inputs[key] = (kc, vc, qkv, anc, ref)
    return _inputs[key]


def identity(R, cap):
    return np.repeat(np.arange(R, dtype=np.uint8)[:, None], cap, axis=1)


@pytest.mark.parametrize("R,H,cap,pos", CASES)
def test_reads_the_ancestors_rows_and_appends_to_its_own(eng, R, H, cap, pos):
    d = 64 * H
    kc, vc, qkv, anc, ref = inputs(R, H, cap, pos)
    out, kc2, vc2 = eng.dbg_self_attention_long_gather(qkv, kc, vc, pos, anc, bf16=True)
    err = np.abs(out - ref).max()
    print(f"rows {R} H {H} cap {cap} pos {pos}: max |delta| {err:.2e}")
    # positions > pos hold 1e30: one of them read as a key or a value would give inf / nan or a huge output
    assert np.isfinite(out).all()
    assert err < BAR
    # exactly the cells [r][pos] change, to the roundings of the new k and v
    want_k, want_v = kc.copy(), vc.copy()
    want_k[:, pos] = bf16_round(qkv[:, d:2 * d])
    want_v[:, pos] = bf16_round(qkv[:, 2 * d:])
    assert np.array_equal(bits(kc2), bits(want_k)) and np.array_equal(bits(vc2), bits(want_v))


@pytest.mark.parametrize("R,H,cap,pos", [(1, 2, 160, 32), (5, 6, 160, 65), (125, 6, 448, 447), (128, 2, 160, 65)])
def test_the_identity_table_gives_the_bits_of_the_ungathered_bf16_kernel(eng, R, H, cap, pos):
    kc, vc, qkv, _, _ = inputs(R, H, cap, pos)
    got = eng.dbg_self_attention_long_gather(qkv, kc, vc, pos, identity(R, cap), bf16=True)
    want = eng.dbg_self_attention_long(qkv, kc, vc, pos, bf16=True)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))


@pytest.mark.parametrize("cap,pos", [(160, 65), (448, 447)])
def test_an_entry_past_the_rows_reads_the_last_row(eng, cap, pos):
    R, H = 5, 6
    kc, vc, qkv, anc, _ = inputs(R, H, cap, pos)
    wild = anc.copy()
    wild[wild == R - 1] = np.resize(np.array([5, 6, 127, 128, 200, 255], np.uint8), int((wild == R - 1).sum()))
    assert wild[:, :pos].max() >= R
    got = eng.dbg_self_attention_long_gather(qkv, kc, vc, pos, wild, bf16=True)
    want = eng.dbg_self_attention_long_gather(qkv, kc, vc, pos, anc, bf16=True)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))


def test_launcher_refusals_return_a_status(eng, pkg):
    def refused(R, H, cap, pos, table=True):
        L = pkg.lib()
        r_, h_, c_ = max(min(R, 129), 1), max(H, 1), max(min(cap, 448), 1)
        k = np.zeros((r_, c_, h_ * 64), np.float32)
        v = k.copy()
        out = np.zeros((r_, h_ * 64), np.float32)
        q = np.zeros((r_, 3 * h_ * 64), np.float32)
        anc = np.zeros((r_, c_), np.uint8)
        fp = lambda a: a.ctypes.data_as(POINTER(c_float))
        rc = L.wt_dbg_self_attention_long_gather_bf16(eng.handle, R, H, cap, pos, fp(q), fp(k), fp(v), fp(out),
                                                      anc.ctypes.data_as(POINTER(c_uint8)) if table else None)
        return pkg.STATUS_NAMES.get(rc)

    assert refused(3, 2, 160, -1) == INVALID
    assert refused(3, 2, 160, 160) == INVALID
    assert refused(3, 2, 449, 10) == INVALID
    assert refused(0, 2, 160, 40) == INVALID
    assert refused(129, 2, 32, 4) == INVALID
    assert refused(3, 0, 160, 40) == INVALID
    assert refused(3, 2, 160, 40, table=False) == INVALID
    assert refused(128, 2, 32, 31) == "WT_OK"
    # the engine is unharmed
    kc, vc, qkv, anc, ref = inputs(5, 6, 160, 65)
    out, _, _ = eng.dbg_self_attention_long_gather(qkv, kc, vc, 65, anc, bf16=True)
    assert np.abs(out - ref).max() < BAR
