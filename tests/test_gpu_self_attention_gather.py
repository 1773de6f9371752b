"""The gathered form of self_attention_long (k_attention.hip) through its debug tap against float64
numpy: up to 128 rows share one cache, and row r reads key k < pos from cache row min(anc[r][k], rows - 1).  Positions
are the edges of the 16-key groups and of the 64-key load rounds and the last row of either cache size.  Without the
feature the tap does not exist and every test here fails."""
from ctypes import POINTER, c_float, c_uint8

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 1e-5  # the project's bar for this computation (test_gpu_self_attention_long.py, standard-normal inputs)
INVALID = "WT_ERR_INVALID_ARG"
POSITIONS = [0, 1, 15, 16, 17, 63, 64, 65, 159]
# (rows, H, cap, pos): every position at 3 rows and either head count, the last row of the long cache, and 128 rows
CASES = ([(3, H, 160, pos) for H in (2, 6) for pos in POSITIONS] + [(3, 2, 448, 447), (3, 6, 448, 447)] +
         [(128, 2, 160, 65), (128, 6, 448, 447)])


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


def gathered(cache, anc, r, pos):
    """Row r's keys 0 .. pos - 1 as the kernel must read them: [pos][d]."""
    rows = cache.shape[0]
    src = np.minimum(anc[r, :pos].astype(np.int64), rows - 1)
    return cache[src, np.arange(pos)]


_inputs = {}


def inputs(R, H, cap, pos):
    """Caches with positions < pos standard normal and positions >= pos filled with 1e30, the new rows, a random table
    (entries at k >= pos hold 255: they must not be read) and the float64 result."""
    key = (R, H, cap, pos)
    if key not in _inputs:
        rng = np.random.default_rng(cap * 1000 + pos * 10 + H + 7 * R)
        d = 64 * H
        kc = np.full((R, cap, d), 1e30, np.float32)
        vc = np.full((R, cap, d), 1e30, np.float32)
        kc[:, :pos] = rng.standard_normal((R, pos, d))
        vc[:, :pos] = rng.standard_normal((R, pos, d))
        qkv = rng.standard_normal((R, 3 * d)).astype(np.float32)
        anc = np.full((R, cap), 255, np.uint8)
        anc[:, :pos] = rng.integers(0, R, size=(R, pos))
        ref = np.zeros((R, d))
        for r in range(R):
            k = np.concatenate([gathered(kc, anc, r, pos), qkv[r:r + 1, d:2 * d]]).astype(np.float64)
            v = np.concatenate([gathered(vc, anc, r, pos), qkv[r:r + 1, 2 * d:]]).astype(np.float64)
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                ref[r, sl] = attn_ref(qkv[r:r + 1, sl].astype(np.float64), k[:, sl], v[:, sl])[0]
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
    out, kc2, vc2 = eng.dbg_self_attention_long_gather(qkv, kc, vc, pos, anc)
    err = np.abs(out - ref).max()
    print(f"rows {R} H {H} cap {cap} pos {pos}: max |delta| {err:.2e}")
    # positions > pos hold 1e30: one of them read as a key or a value would give inf / nan or a huge output
    assert np.isfinite(out).all()
    assert err < BAR
    # exactly the cells [r][pos] change
    want_k, want_v = kc.copy(), vc.copy()
    want_k[:, pos] = qkv[:, d:2 * d]
    want_v[:, pos] = qkv[:, 2 * d:]
    assert np.array_equal(kc2, want_k) and np.array_equal(vc2, want_v)


@pytest.mark.parametrize("R,H,cap,pos", [(3, 2, 160, 0), (3, 6, 160, 17), (3, 6, 160, 65), (3, 2, 448, 447), (128, 6, 160, 159)])
def test_the_identity_table_gives_the_bits_of_the_ungathered_kernel(eng, R, H, cap, pos):
    kc, vc, qkv, _, _ = inputs(R, H, cap, pos)
    got = eng.dbg_self_attention_long_gather(qkv, kc, vc, pos, identity(R, cap))
    want = eng.dbg_self_attention_long(qkv, kc, vc, pos)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("cap,pos", [(160, 65), (448, 447)])
def test_an_entry_past_the_rows_reads_the_last_row(eng, cap, pos):
    R, H = 3, 2
    kc, vc, qkv, anc, _ = inputs(R, H, cap, pos)
    wild = anc.copy()
    wild[wild == R - 1] = np.resize(np.array([3, 4, 127, 128, 200, 255], np.uint8), int((wild == R - 1).sum()))
    assert wild[:, :pos].max() >= R
    got = eng.dbg_self_attention_long_gather(qkv, kc, vc, pos, wild)
    want = eng.dbg_self_attention_long_gather(qkv, kc, vc, pos, anc)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("H,cap,pos", [(2, 160, 65), (6, 448, 447)])
def test_a_row_is_bit_identical_alone_or_among_128(eng, H, cap, pos):
    R = 128
    kc, vc, qkv, anc, _ = inputs(R, H, cap, pos)
    out, _, _ = eng.dbg_self_attention_long_gather(qkv, kc, vc, pos, anc)
    for r in (0, 77, 127):
        # the row's history laid out in a cache of its own
        k1 = np.full((1, cap, 64 * H), 1e30, np.float32)
        v1 = k1.copy()
        k1[0, :pos] = gathered(kc, anc, r, pos)
        v1[0, :pos] = gathered(vc, anc, r, pos)
        alone, _, _ = eng.dbg_self_attention_long_gather(qkv[r:r + 1], k1, v1, pos, np.zeros((1, cap), np.uint8))
        assert np.array_equal(alone[0], out[r])
        plain, _, _ = eng.dbg_self_attention_long(qkv[r:r + 1], k1, v1, pos)
        assert np.array_equal(plain[0], out[r])


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
        rc = L.wt_dbg_self_attention_long_gather(eng.handle, R, H, cap, pos, fp(q), fp(k), fp(v), fp(out),
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
    kc, vc, qkv, anc, ref = inputs(3, 2, 160, 64)
    out, _, _ = eng.dbg_self_attention_long_gather(qkv, kc, vc, 64, anc)
    assert np.abs(out - ref).max() < BAR
