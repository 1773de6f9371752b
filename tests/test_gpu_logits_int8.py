"""GPU (-m gpu): the int8 dynamic-range logits head (option logits_int8): the kernel through
dbg_dec_logits_i8 (quantised rows, logits bit for bit, records), the engine through the option."""
import numpy as np
import pytest

import logits_int8_ref as ref
from test_gpu_decoder_step import argmax_last, check_records, eng, ln64  # noqa: F401 (eng: the micro engine fixture)

pytestmark = pytest.mark.gpu

_ROWS_BLOCKS = [(1, 0), (31, 256), (33, 32), (128, 32)]


def check_head(pkg, lg, rec, qx, sx, E, M):
    """(b) logits bit for bit from the kernel's own rows and the host table, (c) records = the fold of those logits"""
    qw, sw = pkg.quantize_rows_i8(E)
    assert np.array_equal(lg[:M].view(np.uint32), ref.logits(qx, sx, qw, sw).view(np.uint32))
    check_records(lg, rec, M, E.shape[0])


@pytest.mark.parametrize("lnmode", [0, 3])
@pytest.mark.parametrize("K,V", [(128, 1000), (384, 51865), (512, 51865)])
def test_logits_i8_rows_logits_records(pkg, eng, K, V, lnmode):
    rng = np.random.default_rng(K * 100003 + V + lnmode)
    xin = (rng.standard_normal((128, K)) * 2 + 0.5).astype(np.float32)
    xpart = rng.standard_normal((128, K)).astype(np.float32) if lnmode == 3 else None
    g_, b_ = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    E = (rng.standard_normal((V, K)) / 16).astype(np.float32)
    ln = ln64(xin + xpart if xpart is not None else xin, g_, b_)
    q_ref, s_ref = ref.quantize_rows(ln.astype(np.float32))
    # the fp32 LayerNorm is a few 1e-6 (relative) off the float64 one, times 127: inside 2e-3 of a boundary it may round either way
    near = ref.boundary_distance(ln) < 2e-3
    assert near.mean() < 0.01  # (a condition on the inputs: about 0.4 % expected)
    for M, blocks in (_ROWS_BLOCKS if V < 4096 else _ROWS_BLOCKS[int(lnmode == 3)::2]):
        xp = None if xpart is None else xpart[:M]
        lg, rec, qx, sx = eng.dbg_dec_logits_i8(xin[:M], g_, b_, E, xpart=xp, blocks=blocks)
        ulps = np.abs(sx.view(np.int32).astype(np.int64) - s_ref[:M].view(np.int32))
        assert ulps.max() <= 4
        diff = np.abs(qx.astype(np.int32) - q_ref[:M])
        assert diff.max() <= 1 and not diff[~near[:M]].any()
        check_head(pkg, lg, rec, qx, sx, E, M)
        _, rec_only, _, _ = eng.dbg_dec_logits_i8(xin[:M], g_, b_, E, xpart=xp, blocks=blocks, want_logits=False)
        assert np.array_equal(rec_only, rec)


@pytest.mark.parametrize("lnmode", [0, 3])
def test_logits_i8_edge_rows(pkg, eng, lnmode):
    """40 rows (rows 32 .. 39 repeat rows 0 .. 7) on 32 blocks: gridDim.x = 16, a wavefront's tiles are 64 apart.  First:
    duplicate rows of E planted as a row's maximum wherever two columns meet.  Second, with ln_b = 0 and one gain 1e4 times
    the others: every row's other elements quantise to 0, and a constant row normalises to exactly 0 (scale 0, every logit 0)."""
    rng = np.random.default_rng(90 + lnmode)
    K, V, M, blocks, gx = 384, 51865, 40, 32, 16
    ties = {0: [5 * 32 + 3, 5 * 32 + 17], 1: [9 * 32 + 7, 9 * 32 + 31, 10 * 32 + 0], 2: [(7 + gx) * 32 + 2, 7 * 32 + 30],
            3: [3 * 32 + 10, (3 + 4 * gx) * 32 + 5], 4: [51840, 51852, 51862], 5: [0, V - 1]}
    xin = (rng.standard_normal((M, K)) * 2 + 0.5).astype(np.float32)
    xpart = rng.standard_normal((M, K)).astype(np.float32) if lnmode == 3 else None
    xin[32:] = xin[:8]
    x = xin
    if xpart is not None:
        xpart[32:] = xpart[:8]
        x = xin + xpart
    g_, b_ = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    E = (rng.standard_normal((V, K)) / 16).astype(np.float32)
    ln = ln64(x, g_, b_)
    for r, cols in ties.items():
        E[cols] = (ln[r] / 16).astype(np.float32)
    lg, rec, qx, sx = eng.dbg_dec_logits_i8(xin, g_, b_, E, xpart=xpart, blocks=blocks)
    check_head(pkg, lg, rec, qx, sx, E, M)
    zero = np.zeros(M, np.int32)
    ids, _, _ = eng.dbg_select_token(rec[:M], np.zeros((M, 32), np.int64), 4, zero, zero, -1, stop_at_eot=False)
    for r, cols in ties.items():
        for rr in (r, r + 32):
            row = lg[rr]
            assert (row[cols] == row[cols[0]]).all() and row[cols[0]] == row.max(), (rr, cols)
            assert ids[rr, 5] == max(cols), (rr, cols, ids[rr, 5])
    assert all(ids[rr, 5] == argmax_last(lg[rr]) for rr in range(M))

    g_ = np.ones(K, np.float32)
    g_[100] = 1.0e4
    xin[:, 100] = x.mean(axis=1) + 3.0 * x.std(axis=1) - (0.0 if xpart is None else xpart[:, 100])  # |z| ~ 3 there
    xin[9] = 0.75
    if xpart is not None:
        xpart[9] = -0.25  # the row's sum is the same exact value everywhere
    lg, rec, qx, sx = eng.dbg_dec_logits_i8(xin, g_, np.zeros(K, np.float32), E, xpart=xpart, blocks=blocks)
    check_head(pkg, lg, rec, qx, sx, E, M)
    others = np.delete(np.arange(M), 9)
    assert (np.abs(qx[others, 100]) == 127).all() and np.count_nonzero(qx[others]) == M - 1
    assert sx[9] == 0.0 and not qx[9].any() and not lg[9].any()
    last_valid = np.minimum(np.arange((V + 31) // 32) * 32 + 31, V - 1)
    assert np.array_equal(rec[9], (np.uint64(0x80000000) << np.uint64(32)) | last_valid.astype(np.uint64))


# ------------------------------------------------------------------------------------------- the engine, through the option ---
@pytest.fixture(scope="module", params=[("micro", 0), ("micro", 1), ("tiny", 0)], ids=["micro", "micro-bf16", "tiny"])
def model(request, pkg, assets):
    from wtw import read_wtw
    arch, bf16 = request.param
    prefix, vocab = assets(arch)
    e = pkg.Engine(prefix, vocab, True)
    e.set_option("stop_at_eot", 0)
    e.set_option("bf16", bf16)
    if arch == "micro":
        e.set_prompt([3, 5, 7, 11])  # the micro vocabulary (1024) has no special ids
    e.set_option("max_tokens", 9)    # a four-id prompt and 6 argmax steps
    mel = np.random.default_rng(37).uniform(-1.0, 1.5, size=(2,) + e.mel_shape).astype(np.float32)
    yield e, read_wtw(prefix + ".wtw"), mel
    e.close()


def test_engine_head_bound_and_consistency(pkg, model):
    """The option takes 0 and 1 alone.  fp32 storage: every step's logits within the spec's worst case + the fp32 path's
    1e-4 of the float64 decoder's.  Both storage modes: they differ from the default head's, the
    ids are the tie-rule argmax of the logits returned, and option 0 gives the default head's results back bit for bit."""
    e, (dims, tensors), mel = model
    bf16 = e.get_option("bf16")
    for bad in (2, -1):
        with pytest.raises(pkg.WtError) as err:
            e.set_option("logits_int8", bad)
        assert err.value.code == 1 and e.get_option("logits_int8") == 0
    try:
        ids0, n0, enc, lg0 = e.encdec_debug_batch(mel, steps_cap=6)
        assert list(n0) == [10, 10]
        e.set_forced_ids(ids0)  # both heads see the same rows
        e.set_option("logits_int8", 1)
        assert e.get_option("logits_int8") == 1
        _, _, _, lg_on = e.encdec_debug_batch(mel, steps_cap=6)
        e.set_forced_ids(None)
        ids1, n1, _, lg1 = e.encdec_debug_batch(mel, steps_cap=6)
        e.set_option("logits_int8", 0)
        ids2, _, _, lg2 = e.encdec_debug_batch(mel, steps_cap=6)
    finally:
        e.set_forced_ids(None)
        e.set_option("logits_int8", 0)
    assert np.array_equal(ids2, ids0) and np.array_equal(lg2.view(np.uint32), lg0.view(np.uint32))
    E = np.asarray(tensors["decoder.token_embedding.weight"], np.float64)
    for b in range(2):
        for s in range(6):
            assert (lg_on[b, s] != lg0[b, s]).any(), (b, s)
            assert ids1[b, 4 + s] == argmax_last(lg1[b, s]), (b, s)
        if not bf16:
            lg64, ln = ref.decoder_rows(dims, tensors, list(ids0[b, :9]), enc[b])
            err, bar = np.abs(lg_on[b] - lg64[3:]), ref.worst_case(ln[3:], E) + 1e-4
            print(f"clip {b}: largest share of the bar {(err / bar).max():.3f}")
            assert (err <= bar).all(), (b, (err / bar).max())
