"""GPU (-m gpu): the tail of every greedy decoder step, kernel by kernel, through the debug taps of include/wt_debug.h:
fc2 as a K-split residual GEMM (dec_gemm<kProNone, kDecResid> with ksplit = 2), the LayerNorm prologue of the next
GEMM over every row source (xin, xin + xpart, embedding rows of several positions), the persistent logits kernel with
the final LayerNorm and its per-tile argmax records, and select_token.  References are float64 numpy; the records are
checked against a host fold of the kernel's own logits, with exact ties planted wherever the records of two columns
meet ("The greedy step's tail")."""
import numpy as np
import pytest
from scipy.special import erf

pytestmark = pytest.mark.gpu

LOGIT_GUARD = 1.0e30            # the taps' fill of the logits buffer (Engine.dbg_dec_logits)
REC_GUARD = 0xA5A5A5A5A5A5A5A5  # ... and of the records buffer


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def gelu(x):
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def rel_err(a, ref):
    return np.abs(a - ref).max() / max(1e-30, np.abs(ref).max())


def bf16_round(x):
    """round-to-nearest-even to bf16, returned as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def argmax_last(x):
    x = np.asarray(x)
    return int(len(x) - 1 - np.argmax(x[::-1]))


def ln64(x, g, b):
    x = np.asarray(x, np.float64)
    return (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5) * g + b


def ln_product_ref(ln, b_, W, bf16):
    """Reference of LayerNorm rows ln [M][K] (float64) contracted with W [N][K]: (ref, slack).  fp32 form: ln . W^T, no
    slack.  bf16 form: the kernel rounds its fp32 LayerNorm to bf16 in registers and W is stored as bf16; products are
    exact and accumulated in fp32, so ref = bf16(ln) . bf16(W)^T.  An element within 2^-20 (|z g| + |b|) of a bf16
    rounding boundary (well above the fp32 LayerNorm's own error of a few ulps) may round either way in the kernel,
    which moves its row's outputs by up to the distance of the two candidates times |W[:, k]|: that is the slack."""
    if not bf16:
        return ln @ W.astype(np.float64).T, 0.0
    Wb = bf16_round(W).astype(np.float64)
    ref = bf16_round(ln.astype(np.float32)).astype(np.float64) @ Wb.T
    win = 2.0 ** -20 * (np.abs(ln - b_) + np.abs(b_))
    lo = bf16_round((ln - win).astype(np.float32)).astype(np.float64)
    hi = bf16_round((ln + win).astype(np.float32)).astype(np.float64)
    slack = np.zeros(ref.shape)
    for r, k in zip(*np.nonzero(hi != lo)):
        slack[r] += (hi[r, k] - lo[r, k]) * np.abs(Wb[:, k])
    return ref, slack


def check_ln_gemm(Y, ln, b_, W, bias, gelu_on, bf16):
    """Y = act(LN . W^T + bias) against float64: fp32 accumulation behind an fp32 LayerNorm, < 5e-6 of the largest
    output (test_gpu_kernels.py); the bf16 form on its rounded operands at the same bar plus the slack of
    ln_product_ref (GELU's slope stays below 1.13)."""
    ref, slack = ln_product_ref(ln, b_, W, bf16)
    ref = ref + bias
    if gelu_on:
        ref, slack = gelu(ref), 1.13 * slack
    err = np.abs(Y - ref)
    bar = 5e-6 * np.abs(ref).max() + slack
    assert (err <= bar).all(), (err.max(), (err - bar).max())


def ordered_keys(v):
    """the kernel's ordered_bits: v + 0 (-0 -> +0), then sign-magnitude to unsigned order"""
    u = (np.asarray(v, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def fold_records(logits, V):
    """Host fold of logits [M][V] into per-tile records: the largest ordered key over the tile's columns < V, then the
    LARGEST column among equals; record = key << 32 | column."""
    M, T = logits.shape[0], (V + 31) // 32
    keys = np.zeros((M, T * 32), np.uint64)
    keys[:, :V] = ordered_keys(logits[:, :V])
    keys = keys.reshape(M, T, 32)
    kmax = keys.max(axis=2)
    valid = (np.arange(T * 32) < V).reshape(T, 32)
    hit = (keys == kmax[:, :, None]) & valid[None]
    col = np.arange(T)[None, :] * 32 + 31 - np.argmax(hit[:, :, ::-1], axis=2)
    return (kmax << np.uint64(32)) | col.astype(np.uint64)


def check_records(logits, records, M, V):
    """records[:M] are the fold of the kernel's own logits, bit for bit; both guard rows are untouched"""
    assert np.array_equal(records[:M], fold_records(logits[:M], V))
    assert (records[M] == np.uint64(REC_GUARD)).all()
    assert (logits[M] == np.float32(LOGIT_GUARD)).all()


def select_ref(records, ids, pos, n_ids, finished, eot, stop_at_eot, keep_ids):
    """The greedy step (whisper.cpp:392-399) as select_token states it: the largest record (ordered key, then column)
    gives the token; ids[b][pos + 1] receives it unless the rows are given (keep_ids); a clip that has not finished
    counts it (n_ids = pos + 2) and finishes on EOT when stop_at_eot."""
    ids, n_ids, finished = ids.copy(), n_ids.copy(), finished.copy()
    tok = (records.max(axis=1) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    for b in range(records.shape[0]):
        if not keep_ids:
            ids[b, pos + 1] = tok[b]
        if not finished[b]:
            n_ids[b] = pos + 2
            if stop_at_eot and tok[b] == eot:
                finished[b] = 1
    return ids, n_ids, finished


# ------------------------------------------------------------------------------------------------ K-split fc2 ---
@pytest.mark.parametrize("bf16", [False, True], ids=["planes", "bf16"])
@pytest.mark.parametrize("K", [512, 1536, 2048])
@pytest.mark.parametrize("N", [128, 384, 512])
def test_fc2_ksplit_halves(eng, N, K, bf16):
    """fc2 with fc2_ksplit = 2 (the engine's default): the blocks of the first K-half finish Y = R + b + X[:, :K/2] W^T,
    those of the second leave the raw partial X[:, K/2:] W^T in `part`; only half 0 carries bias and residual, R is read
    and never written, two launches agree bit for bit.  Budget: each half is an ordinary dec_gemm contraction, < 3e-6 of
    its largest element (test_gpu_kernels.py); Y + part is summed in float64 here, so the whole stays < 3e-6 of
    max |R + b + X W^T|.  A bias added by both halves is off by |b| ~ 1."""
    rng = np.random.default_rng(N * 7 + K + int(bf16))
    rnd = bf16_round if bf16 else (lambda a: a)
    Xall = rng.standard_normal((128, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / 16).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    Rall = rng.standard_normal((128, N)).astype(np.float32)
    Wd = rnd(W).astype(np.float64)
    for M, B in ((1, 1), (5, 5), (32, 32), (33, 33), (64, 32), (100, 25), (128, 32)):
        X, R = Xall[:M], Rall[:M]
        Xd = rnd(X).astype(np.float64)
        h0 = Xd[:, :K // 2] @ Wd[:, :K // 2].T
        h1 = Xd[:, K // 2:] @ Wd[:, K // 2:].T
        Y, part, R_back = eng.dbg_dec_gemm_ksplit(X, W, bias, R, B=B, bf16=bf16)
        assert np.array_equal(R_back, R), M
        assert rel_err(part, h1) < 3e-6, (M, rel_err(part, h1))
        base = R.astype(np.float64) + bias
        assert rel_err(Y, base + h0) < 3e-6, (M, rel_err(Y, base + h0))
        assert rel_err(Y.astype(np.float64) + part, base + Xd @ Wd.T) < 3e-6, M
        Y2, part2, _ = eng.dbg_dec_gemm_ksplit(X, W, bias, R, B=B, bf16=bf16)
        assert np.array_equal(Y2, Y) and np.array_equal(part2, part), M  # fixed reduction order, no atomics


# ------------------------------------------------------------------------- LayerNorm prologue, every row source ---
@pytest.mark.parametrize("bf16", [False, True], ids=["planes", "bf16"])
@pytest.mark.parametrize("M,B,K,N", [(33, 33, 384, 1152), (64, 32, 512, 512), (97, 97, 128, 512), (128, 32, 384, 384)])
def test_ln_prologue_pending_partial(eng, M, B, K, N, bf16):
    """LNMODE 3, the LayerNorm after a K-split fc2: x = xin + xpart in fp32; block 0 stores x to xout for EVERY row
    group (rows 64.. are the second group of two 32-row tiles), the guard row stays; Y matches the float64
    LN(xin + xpart) . W^T + b with and without GELU (budget: check_ln_gemm).  LNMODE 0 over the same sum stores
    nothing and gives the same Y."""
    rng = np.random.default_rng(M + K + N + int(bf16))
    xin = (rng.standard_normal((M, K)) * 2 + 0.5).astype(np.float32)
    xpart = rng.standard_normal((M, K)).astype(np.float32)
    g_, b_ = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    W = (rng.standard_normal((N, K)) / 16).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    x = xin + xpart  # fp32, as the kernel sums
    ln = ln64(x, g_, b_)
    guard = rng.standard_normal((M + 1, K)).astype(np.float32)
    for gelu_on in (False, True):
        Y, xout = eng.dbg_dec_ln_gemm_rows(W, bias, g_, b_, xin=xin, xpart=xpart, B=B, gelu=gelu_on, bf16=bf16, xout=guard)
        bad = np.nonzero((xout[:M] != x).any(axis=1))[0]
        assert bad.size == 0, f"xout rows not completed: {bad[:8]} ..."
        assert np.array_equal(xout[M], guard[M])
        check_ln_gemm(Y, ln, b_, W, bias, gelu_on, bf16)
    Y0, xout0 = eng.dbg_dec_ln_gemm_rows(W, bias, g_, b_, xin=x, B=B, bf16=bf16, xout=guard)
    assert np.array_equal(xout0, guard)
    check_ln_gemm(Y0, ln, b_, W, bias, False, bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["planes", "bf16"])
@pytest.mark.parametrize("n_p,B,pos,K,N", [(2, 64, 27, 384, 1152), (3, 33, 5, 512, 384), (4, 32, 0, 384, 1152),
                                           (4, 25, 28, 128, 384)])
def test_ln_prologue_embedding_rows(eng, n_p, B, pos, K, N, bf16):
    """LNMODE 2, layer 0 of a pass over n_p positions: row p * B + b = tok_emb[ids[b][pos + p]] + pos_emb[pos + p], stored
    to xout bit for bit (guard row untouched) and normalised (budget: check_ln_gemm); ids outside [0, n_vocab) are
    clamped to the table's ends, as load_row promises.  The ids of a clip differ from position to position, and the
    ids around the pass's window are garbage the kernel must not read."""
    rng = np.random.default_rng(n_p * 1000 + B + pos + int(bf16))
    V, n_ctx, stride = 300, 32, 32
    M = n_p * B
    tok = rng.standard_normal((V, K)).astype(np.float32)
    pe = rng.standard_normal((n_ctx, K)).astype(np.float32)
    ids = rng.integers(-10 ** 9, 10 ** 9, size=(B, stride))
    ids[:, pos:pos + n_p] = rng.integers(0, V, size=(B, n_p))
    ids[0, pos] = -1
    ids[1, pos + n_p - 1] = V
    ids[2, pos + 1] = 10 ** 12
    ids[3, pos] = -(10 ** 12)
    ids[4, pos + n_p - 1] = V - 1
    rows = np.clip(ids[:, pos:pos + n_p], 0, V - 1)  # [B][n_p]
    x = tok[rows.T.reshape(-1)] + pe[np.repeat(np.arange(pos, pos + n_p), B)]  # row p * B + b, fp32 as the kernel adds
    g_, b_ = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    W = (rng.standard_normal((N, K)) / 16).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    guard = rng.standard_normal((M + 1, K)).astype(np.float32)
    Y, xout = eng.dbg_dec_ln_gemm_rows(W, bias, g_, b_, ids=ids, pos=pos, tok_emb=tok, pos_emb=pe, M=M, bf16=bf16,
                                       xout=guard)
    bad = np.nonzero((xout[:M] != x).any(axis=1))[0]
    assert bad.size == 0, f"embedding rows wrong: {bad[:8]} ..."
    assert np.array_equal(xout[M], guard[M])
    check_ln_gemm(Y, ln64(x, g_, b_), b_, W, bias, False, bf16)


def test_ln_row_statistics_edges(eng):
    """The row statistics (row_stats, shared by dec_gemm's LayerNorm prologue and the persistent logits kernel), read
    through an identity contraction, which returns the normalised row itself (a 22-bit plane split relative to the
    largest element of a k-slice: 2.4e-7 of the row's largest |LN|):
      * ordinary rows, under LN gains N(0, 1) and under gains spanning 1e-3 .. 1e3: < 5e-6 of the row's largest |LN|;
      * rows 1e3 + N(0, 1): the fp32 mean of values near 1e3 is off by ~1e-4 (a few 1e-3 at worst: lane sums of 48
        terms near 5e4), which shifts the normalised row by that over sigma = 1, bar 1e-2 of the row's largest |LN|;
        a one-pass variance (E[x^2] - mean^2 of terms near 1e6 in fp32) loses ~0.1 of sigma^2;
      * constant rows 3.0, -0.75 and 0.0, whose fp32 sums are exact: the mean is exact, x - mean is 0 and the
        normalised row is exactly ln_b (values on a 1/8 grid: exact through the planes).
    Rows 33 and 38 put offset rows into the second 32-row tile."""
    rng = np.random.default_rng(11)
    K, M, V = 384, 40, 1000
    x = (rng.standard_normal((M, K)) * 2 + 0.5).astype(np.float32)
    offset = [0, 1, 2, 3, 4, 5, 6, 7, 33, 38]
    const = [8, 9, 10]
    x[offset] = (1e3 + rng.standard_normal((len(offset), K))).astype(np.float32)
    x[8], x[9], x[10] = 3.0, -0.75, 0.0
    ordinary = [r for r in range(M) if r not in offset and r not in const]
    eye = np.eye(K, dtype=np.float32)
    E = np.concatenate([eye, (rng.standard_normal((V - K, K)) / 16).astype(np.float32)])
    b_ = (rng.integers(-32, 33, K) / 8).astype(np.float32)
    g_ = rng.standard_normal(K).astype(np.float32)
    g_wide = (10.0 ** rng.uniform(-3, 3, K) * rng.choice([-1.0, 1.0], K)).astype(np.float32)
    W = (rng.standard_normal((512, K)) / 16).astype(np.float32)
    for g in (g_, g_wide):
        ln = ln64(x, g, b_)
        Y, _ = eng.dbg_dec_ln_gemm_rows(eye, np.zeros(K, np.float32), g, b_, xin=x)
        lg, rec = eng.dbg_dec_logits(x, g, b_, E, blocks=32)
        check_records(lg, rec, M, V)
        for name, out in (("dec_gemm", Y), ("dec_logits_persistent", lg[:M, :K])):
            err, scale = np.abs(out - ln).max(axis=1), np.abs(ln).max(axis=1)
            assert (err[ordinary] <= 5e-6 * scale[ordinary]).all(), (name, (err / scale)[ordinary].max())
            assert (err[offset] <= 1e-2 * scale[offset]).all(), (name, (err / scale)[offset].max())
            for r in const:
                assert np.array_equal(out[r], b_), (name, r)
        # the ordinary and constant rows through an ordinary contraction
        keep = ordinary + const
        Yw, _ = eng.dbg_dec_ln_gemm_rows(W, np.zeros(512, np.float32), g, b_, xin=x[keep])
        assert rel_err(Yw, ln[keep] @ W.astype(np.float64).T) < 5e-6


# ------------------------------------------------------------------- persistent logits with the LayerNorm prologue ---
_ROWS_BLOCKS = [(1, 0), (31, 256), (33, 32), (64, 0), (100, 256), (128, 32)]


@pytest.mark.parametrize("lnmode", [0, 3])
@pytest.mark.parametrize("K,V", [(128, 1000), (384, 51864), (384, 51865), (512, 51865)])
def test_logits_persistent_and_records(eng, K, V, lnmode):
    """dec_logits_persistent<KS, BF, LNMODE 0 | 3>, fp16 planes and bf16: the final LayerNorm of xin (+ xpart), logits
    against E and one (value, column) record per (row, 32-column tile), for 1 .. 128 rows (up to four blockIdx.y row
    tiles) on 512 (default), 256 and 32 resident blocks (at 32 a block walks ~50 tiles; V = 1000 has fewer tiles than
    blocks).  Logits: fp32 < 5e-6 of the largest (behind a LayerNorm), bf16 on its rounded operands (ln_product_ref).
    Records: the host fold of the kernel's own logits, bit for bit, and the same when no logits are written; guard
    rows untouched.  At V >= 51864 each precision takes every other (rows, blocks) pair; the float64 reference is made
    once for 128 rows, fewer rows are its first rows."""
    rng = np.random.default_rng(K * 100003 + V + lnmode)
    xin = (rng.standard_normal((128, K)) * 2 + 0.5).astype(np.float32)
    xpart = rng.standard_normal((128, K)).astype(np.float32) if lnmode == 3 else None
    g_, b_ = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    E = (rng.standard_normal((V, K)) / 16).astype(np.float32)
    ln = ln64(xin + xpart if xpart is not None else xin, g_, b_)
    for bf16 in (False, True):
        ref, slack = ln_product_ref(ln, b_, E, bf16)
        bar = 5e-6 * np.abs(ref).max() + slack
        pairs = _ROWS_BLOCKS if V < 4096 else _ROWS_BLOCKS[int(bf16) ^ int(lnmode == 3)::2]
        for M, blocks in pairs:
            xp = None if xpart is None else xpart[:M]
            lg, rec = eng.dbg_dec_logits(xin[:M], g_, b_, E, xpart=xp, blocks=blocks, bf16=bf16)
            err = np.abs(lg[:M] - ref[:M])
            assert (err <= (bar if np.isscalar(bar) else bar[:M])).all(), (bf16, M, blocks, err.max())
            check_records(lg, rec, M, V)
            _, rec_only = eng.dbg_dec_logits(xin[:M], g_, b_, E, xpart=xp, blocks=blocks, bf16=bf16, want_logits=False)
            assert np.array_equal(rec_only, rec), (bf16, M, blocks)


@pytest.mark.parametrize("bf16", [False, True], ids=["planes", "bf16"])
@pytest.mark.parametrize("lnmode", [0, 3])
def test_logits_tie_rule_across_tiles_and_blocks(eng, lnmode, bf16):
    """Duplicate rows of E give bit-identical logits; planted as a row's maximum they must resolve to the LARGEST column
    (the reference's `>=` scan, whisper.cpp:353) wherever the two columns meet: inside one tile, in adjacent tiles, in
    tiles t and t + gridDim.x (one block, two and three iterations apart), in tiles of different blocks, inside the
    partial last tile (columns 51840 .. 51864), and column 0 against V - 1.  40 rows (two row tiles; rows 32 .. 39
    repeat rows 0 .. 7) on 32 resident blocks: gridDim.x = 16.  The token comes out of select_token."""
    rng = np.random.default_rng(60 + lnmode + 2 * int(bf16))
    K, V, M, blocks = 384, 51865, 40, 32
    gx = min((V + 31) // 32, blocks // ((M + 31) // 32))
    ties = {0: [5 * 32 + 3, 5 * 32 + 17],
            1: [9 * 32 + 7, 9 * 32 + 31, 10 * 32 + 0],
            2: [(7 + gx) * 32 + 2, 7 * 32 + 30],
            3: [3 * 32 + 10, 1000 * 32 + 5],
            4: [51840, 51852, 51862],
            5: [0, V - 1],
            6: [51841, 51863],
            7: [2 * 32 + 0, 2 * 32 + 31, (2 + 3 * gx) * 32 + 0]}
    xin = (rng.standard_normal((M, K)) * 2 + 0.5).astype(np.float32)
    xin[32:] = xin[:8]
    xpart = None
    if lnmode == 3:
        xpart = rng.standard_normal((M, K)).astype(np.float32)
        xpart[32:] = xpart[:8]
    g_, b_ = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    ln = ln64(xin + xpart if xpart is not None else xin, g_, b_)
    E = (rng.standard_normal((V, K)) / 16).astype(np.float32)
    for r, cols in ties.items():
        E[cols] = (ln[r] / 16).astype(np.float32)  # logit ~ |LN row|^2 / 16 ~ 50: far above the random ones
    lg, rec = eng.dbg_dec_logits(xin, g_, b_, E, xpart=xpart, blocks=blocks, bf16=bf16)
    check_records(lg, rec, M, V)
    ids, _, _ = eng.dbg_select_token(rec[:M], np.zeros((M, 32), np.int64), 4, np.zeros(M, np.int32),
                                     np.zeros(M, np.int32), -1, stop_at_eot=False)
    for r, cols in ties.items():
        for rr in (r, r + 32):
            row = lg[rr]
            assert (row[cols] == row[cols[0]]).all() and row[cols[0]] == row.max(), (rr, cols)
            assert np.count_nonzero(row == row.max()) == len(cols), rr
            assert ids[rr, 5] == max(cols), (rr, cols, ids[rr, 5])
    for rr in range(M):
        assert ids[rr, 5] == argmax_last(lg[rr]), rr


@pytest.mark.parametrize("bf16", [False, True], ids=["planes", "bf16"])
def test_logits_zero_rows_tie_everywhere(eng, bf16):
    """LayerNorm gain and shift 0 normalise every row to exactly zero: every logit is +0 (the kernel adds + 0.0f before
    it writes), every column of every tile and block ties, each record is its tile's last column BELOW V (the padding
    columns of the last tile, zero weights, must never be chosen), and select_token returns V - 1."""
    rng = np.random.default_rng(70 + int(bf16))
    K, V, M = 512, 51865, 33
    xin = rng.standard_normal((M, K)).astype(np.float32)
    xpart = rng.standard_normal((M, K)).astype(np.float32)
    E = (rng.standard_normal((V, K)) / 16).astype(np.float32)
    zero = np.zeros(K, np.float32)
    lg, rec = eng.dbg_dec_logits(xin, zero, zero, E, xpart=xpart, bf16=bf16)
    assert (lg[:M] == 0).all() and not np.signbit(lg[:M]).any()
    check_records(lg, rec, M, V)
    T = (V + 31) // 32
    cols = np.minimum(np.arange(T) * 32 + 31, V - 1).astype(np.uint64)
    assert (rec[:M] == ((np.uint64(0x80000000) << np.uint64(32)) | cols)[None]).all()
    ids, _, _ = eng.dbg_select_token(rec[:M], np.zeros((M, 32), np.int64), 0, np.zeros(M, np.int32),
                                     np.zeros(M, np.int32), -1, stop_at_eot=False)
    assert (ids[:, 1] == V - 1).all()


# ------------------------------------------------------------------------------------------------- select_token ---
@pytest.mark.parametrize("B", [1, 64, 128])
@pytest.mark.parametrize("n_tiles", [1, 63, 64, 255, 256, 257, 1621])
def test_select_token(eng, n_tiles, B):
    """select_token on hand-made records: one block of four wavefronts per clip, thread t reads tiles t, t + 256, ...
    The maximum is placed in each wavefront's range and in the last tile; equal keys in two tiles resolve to the larger
    column; a clip with all-zero records gets token 0.  The ids row receives the token even for a finished clip, whose
    n_ids stays; EOT finishes a clip only with stop_at_eot; keep_ids leaves the ids alone but still counts.  Compared
    with select_ref, a short restatement of the rule, and with the planted winners."""
    rng = np.random.default_rng(n_tiles * 131 + B)
    vals = rng.standard_normal((B, n_tiles)).astype(np.float32)
    cols = np.arange(n_tiles)[None, :] * 32 + rng.integers(0, 32, (B, n_tiles))
    want = np.zeros(B, np.int64)
    for b in range(B):
        kind = b % 6
        t = n_tiles - 1
        if kind < 4:
            in_wave = [u for u in range(n_tiles) if (u % 256) // 64 == kind]
            if in_wave:
                t = int(rng.choice(in_wave))
        if kind == 5 and n_tiles > 1:  # the same key in an earlier tile: the later tile's (larger) column wins
            t0 = int(rng.integers(0, n_tiles - 1))
            t = int(rng.integers(t0 + 1, n_tiles))
            vals[b, t0] = 10.0 + b
        vals[b, t] = 10.0 + b
        want[b] = cols[b, t]
    records = (ordered_keys(vals).astype(np.uint64) << np.uint64(32)) | cols.astype(np.uint64)
    if B > 1:
        records[B - 1] = 0
        want[B - 1] = 0
    c_eot = min(1, B - 1)
    eot = int(want[c_eot])
    pos, stride = 13, 32
    ids0 = rng.integers(0, 50000, (B, stride)).astype(np.int64)
    n0 = rng.integers(5, 12, B).astype(np.int32)
    fin0 = rng.integers(0, 2, B).astype(np.int32)
    fin0[c_eot] = 0
    for stop, keep in ((1, 0), (0, 0), (1, 1)):
        ids, n, fin = eng.dbg_select_token(records, ids0, pos, n0, fin0, eot, stop_at_eot=stop, keep_ids=keep)
        e_ids, e_n, e_fin = select_ref(records, ids0, pos, n0, fin0, eot, stop, keep)
        assert np.array_equal(ids, e_ids) and np.array_equal(n, e_n) and np.array_equal(fin, e_fin), (stop, keep)
        if keep:
            assert np.array_equal(ids, ids0)
        else:
            assert np.array_equal(ids[:, pos + 1], want)
            assert np.array_equal(np.delete(ids, pos + 1, axis=1), np.delete(ids0, pos + 1, axis=1))
        assert np.array_equal(n[fin0 == 1], n0[fin0 == 1]) and (n[fin0 == 0] == pos + 2).all()
        assert fin[c_eot] == stop and np.array_equal(fin[fin0 == 1], fin0[fin0 == 1])


# ----------------------------------------------------------------------------- the chained tail at whisper shapes ---
@pytest.mark.parametrize("B", [64, 128])
@pytest.mark.parametrize("d,V", [(384, 51864), (512, 51865)])
def test_chained_tail_whisper_shapes(eng, d, V, B):
    """split fc2 -> final LayerNorm of Y + part with the logits (LNMODE 3) -> select_token, against the float64
    argmax_last(LN(R + b + H W2^T) E^T).  Error bound on every logit: the residual GEMM's 3e-6 of max|x|, carried through
    the LayerNorm by max|g| / sigma_min and into a logit by max_n sum_k |E[n, k]|, plus the logits GEMM's 5e-6 of the
    largest logit.  The token must always be the last maximum of the kernel's own logits, and the float64 one wherever
    the float64 top-2 gap exceeds twice the bound.  The same chain with ksplit = 1 (dec_gemm mode 2, then LNMODE 0)
    agrees within twice the bound."""
    rng = np.random.default_rng(d + V + B)
    H = gelu(rng.standard_normal((B, 4 * d))).astype(np.float32)
    W2 = (rng.standard_normal((d, 4 * d)) / 32).astype(np.float32)
    b2 = (rng.standard_normal(d) * 0.1).astype(np.float32)
    R = rng.standard_normal((B, d)).astype(np.float32)
    g_ = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b_ = (0.1 * rng.standard_normal(d)).astype(np.float32)
    E = (rng.standard_normal((V, d)) / 16).astype(np.float32)
    Y, part, _ = eng.dbg_dec_gemm_ksplit(H, W2, b2, R)
    lg, rec = eng.dbg_dec_logits(Y, g_, b_, E, xpart=part)
    check_records(lg, rec, B, V)
    pos = 10
    ids, _, _ = eng.dbg_select_token(rec[:B], np.zeros((B, 32), np.int64), pos, np.zeros(B, np.int32),
                                     np.zeros(B, np.int32), -1, stop_at_eot=False)
    tok = ids[:, pos + 1]
    assert all(tok[b] == argmax_last(lg[b]) for b in range(B))
    x = R.astype(np.float64) + b2 + H.astype(np.float64) @ W2.astype(np.float64).T
    L = ln64(x, g_, b_) @ E.astype(np.float64).T
    sigma = np.sqrt(x.var(axis=1)).min()
    bound = (3e-6 * np.abs(x).max() * np.abs(g_).max() / sigma * np.abs(E).sum(axis=1).max()
             + 5e-6 * np.abs(L).max())
    err = np.abs(lg[:B] - L).max()
    assert err <= bound, (err, bound)
    top2 = np.sort(L, axis=1)[:, -2:]
    sure = top2[:, 1] - top2[:, 0] > 2 * bound
    assert sure.sum() >= B // 2, sure.sum()
    ref_tok = np.array([argmax_last(L[b]) for b in range(B)])
    assert np.array_equal(tok[sure], ref_tok[sure])
    x1 = eng.dbg_dec_gemm(H, W2, b2, mode=2, R=R)
    lg1, rec1 = eng.dbg_dec_logits(x1, g_, b_, E)
    check_records(lg1, rec1, B, V)
    assert np.abs(lg1[:B] - lg[:B]).max() <= 2 * bound


# ------------------------------------------------------------------------------------------------- engine level ---
@pytest.fixture(scope="module")
def tiny(pkg, assets):
    prefix, vocab = assets("tiny")
    e = pkg.Engine(prefix, vocab, True)
    e.set_option("stop_at_eot", 0)
    yield e
    e.close()


@pytest.mark.parametrize("B", [33, 64])
def test_engine_fc2_ksplit_logits_agree(tiny, B):
    """whisper-tiny (d = 384, fc2 K = 1536) decoded with fc2_ksplit 2 (the default), then with 1 behind the same ids
    (wt_dbg_set_forced_ids): the logits of every step must agree within 1e-4, the fp32 bar every logit is held to
    against the fp64-accumulating oracle (LOGIT_TOL, test_gpu_path.py).  The two forms differ only in where one fp32
    sum per layer is rounded (Y + part against one K-sum): a few ulps of the residual stream, far inside that bar.  They
    must not be bit-identical either: the split form is really taken."""
    e = tiny
    mel = np.random.default_rng(90 + B).uniform(-1.0, 1.5, size=(B,) + e.mel_shape).astype(np.float32)
    assert e.get_option("fc2_ksplit") == 2
    ids2, n2, _, lg2 = e.encdec_debug_batch(mel, want_enc_out=False)
    e.set_forced_ids(ids2)
    try:
        e.set_option("fc2_ksplit", 1)
        ids1, n1, _, lg1 = e.encdec_debug_batch(mel, want_enc_out=False)
    finally:
        e.set_forced_ids(None)
        e.set_option("fc2_ksplit", 2)
    assert np.array_equal(ids1, ids2) and np.array_equal(n1, n2)
    worst = 0.0
    for i in range(lg2.shape[1]):
        dl = float(np.abs(lg1[:, i] - lg2[:, i]).max())
        worst = max(worst, dl)
        assert dl < 1e-4, (i, dl)
    assert worst > 0.0
