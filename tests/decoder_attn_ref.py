"""References, bars and cases for the kernel-by-kernel tests of the decoder attention of the 31-position chain
(DESIGN section 24): self_attention_step, cross_attention_step (through its per-chunk records) and the kProCombine
prologue of dec_gemm.

Three layers:
  * float64 references (self_ref, cross_ref, combine_ref) and the bars derived from the inputs;
  * Emu, a plain float32 numpy emulation of each kernel's arithmetic behind the signatures of the Engine's debug taps
    (fp32 dot products, fp32 exp, the same chunk and merge structure; the order inside a sum is numpy's);
  * the cases of sections A, B and C as functions of a backend `eng` (an Engine, or Emu) and a `margin`: every function
    runs its cases through the backend, asserts err <= margin * bar for every row, head and chunk and returns the
    worst err / bar.  tests/test_gpu_decoder_attention.py runs them on the GPU with margin 1,
    tests/test_decoder_attention_reference.py on Emu with margin 1/4: a correct fp32 kernel can meet the bars."""
import numpy as np

U = 2.0 ** -24        # unit round-off of fp32
SELF_BAR = 1e-5       # self-attention output, unit-variance data (tests/test_gpu_kernels.py)
CROSS_BAR = 2e-5      # cross-attention output, unit-variance data (tests/test_gpu_kernels.py)
GEMM_BAR = 3e-6       # residual decoder GEMM, relative to the largest output (tests/test_gpu_decoder_step.py)
LOG2E = 1.44269504088896340736
EMPTY_M = np.float32(np.float32(-1e30) * np.float32(1.0 / LOG2E))  # the m of an empty chunk as the kernel writes it
GEOMETRY_T = (1, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
GEOMETRY = [(T, c) for T in GEOMETRY_T for c in (1, 2, 4, 8) if c <= T]
COMBINE_ROWS = ((1, 1), (31, 31), (32, 32), (33, 11), (64, 32), (97, 97), (128, 32))  # (M, B): B divides M


def bf16_round(x):
    """round-to-nearest-even to bf16, returned as float32 (NaN stays the quiet NaN)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def bits_equal(a, b):
    a, b = f32(a), f32(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ln64(x, g, b):
    x = np.asarray(x, np.float64)
    return (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5) * g + b


def query_ref(x, g, b, wq, bq):
    """float64 LayerNorm + query projection: q [rows][d]"""
    return ln64(x, g, b) @ np.asarray(wq, np.float64).T + np.asarray(bq, np.float64)


def _worst(err, bar, margin, what, slack=0.0):
    """asserts err <= margin * bar + slack everywhere and returns the worst (err - slack) / bar"""
    err, bar, slack = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bar, np.float64), np.asarray(slack, np.float64))
    if err.size == 0:
        return 0.0
    err = np.maximum(err - slack, 0.0)
    ratio = np.where(err == 0, 0.0, err / np.where(bar > 0, bar, 1e-300))  # a zero bar (q = 0) admits a zero error only
    assert np.all(err <= margin * bar), (what, float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------ float64 references ---
def self_ref(qkv, kc, vc, pos0, npos, bf16):
    """Causal attention of npos new positions over a cache [B][cap][d] (rows p * B + b of qkv [npos * B][3d]).
    Returns out [rows][d] (float64), the expected caches (float32: the appended rows, or their bf16 roundings, and
    nothing else changed), and per (row, head) ds = 65 * 2^-24 * max_j sum_c |q_c k_jc| / 8 and max |v| over the keys
    the row attends."""
    rnd = bf16_round if bf16 else f32
    B, cap, d = kc.shape
    H = d // 64
    q3 = f32(qkv).reshape(npos, B, 3, d)
    kc2, vc2 = rnd(kc).copy(), rnd(vc).copy()
    kc2[:, pos0:pos0 + npos] = rnd(q3[:, :, 1]).transpose(1, 0, 2)
    vc2[:, pos0:pos0 + npos] = rnd(q3[:, :, 2]).transpose(1, 0, 2)
    out = np.zeros((npos, B, H, 64))
    ds, vmax = np.zeros((npos, B, H)), np.zeros((npos, B, H))
    for p in range(npos):
        n = pos0 + p + 1
        K = kc2[:, :n].astype(np.float64).reshape(B, n, H, 64)
        V = vc2[:, :n].astype(np.float64).reshape(B, n, H, 64)
        q = q3[p, :, 0].astype(np.float64).reshape(B, H, 64)
        s = np.einsum("bhc,bnhc->bhn", q, K) / 8
        w = np.exp(s - s.max(-1, keepdims=True))
        w /= w.sum(-1, keepdims=True)
        out[p] = np.einsum("bhn,bnhc->bhc", w, V)
        ds[p] = 65 * U * np.einsum("bhc,bnhc->bhn", np.abs(q), np.abs(K)).max(-1) / 8
        vmax[p] = np.abs(V).max(axis=(1, 3))
    return out.reshape(npos * B, d), kc2, vc2, ds.reshape(npos * B, H), vmax.reshape(npos * B, H)


def chunk_bounds(T, chunks):
    """[lo, hi) of every key chunk as the kernel cuts them; hi <= lo is an empty chunk"""
    per = (T + chunks - 1) // chunks
    return [(c * per, min(T, c * per + per)) for c in range(chunks)]


def chunk_stats(s, V, T, chunks):
    """Per-chunk softmax statistics of scores s [..., T] (natural-log units) against values V [..., T][64] (leading axes
    broadcast): mx, lse [..., chunks], mean [..., chunks][64], empty [chunks]"""
    lead = s.shape[:-1]
    mx, lse = np.zeros(lead + (chunks,)), np.full(lead + (chunks,), -np.inf)
    mean = np.zeros(lead + (chunks, 64))
    empty = np.zeros(chunks, bool)
    for c, (lo, hi) in enumerate(chunk_bounds(T, chunks)):
        if hi <= lo:
            empty[c] = True
            continue
        sc = s[..., lo:hi]
        mx[..., c] = sc.max(-1)
        e = np.exp(sc - mx[..., c, None])
        l = e.sum(-1)
        lse[..., c] = mx[..., c] + np.log(l)
        mean[..., c, :] = (e[..., None] * V[..., lo:hi, :]).sum(-2) / l[..., None]
    return mx, lse, mean, empty


def merge_chunks(lse, mean):
    """(lse [..., chunks], mean [..., chunks][64]) -> attention over all keys [..., 64]; an empty chunk has lse = -inf"""
    w = np.exp(lse - lse.max(-1, keepdims=True))
    return (w[..., None] * mean).sum(-2) / w.sum(-1)[..., None]


def attention_ref(s, V):
    """unchunked softmax(s) . V"""
    w = np.exp(s - s.max(-1, keepdims=True))
    return (w[..., None] * V).sum(-2) / w.sum(-1)[..., None]


def cross_ref(x, g, b, wq, bq, kc, vc, chunks, nq, bf16, dq=None):
    """float64 reference of cross_attention_step: per (position p, clip, head, chunk) mx, lse, mean, and the combined
    output; ds per chunk = 65 * 2^-24 * max_j sum_c |q_c k_jc| / 8 (+ max_j sum_c dq_c |k_jc| / 8 when the case gives an
    absolute bound dq [rows][d] on the query's own error), vmax = max |v| of the chunk."""
    rnd = bf16_round if bf16 else f32
    B, H, T, _ = kc.shape
    K, V = rnd(kc).astype(np.float64), rnd(vc).astype(np.float64)
    q = query_ref(x, g, b, wq, bq).reshape(nq, B, H, 64)
    s = np.einsum("pbhc,bhtc->pbht", q, K) / 8
    sa = np.einsum("pbhc,bhtc->pbht", np.abs(q), np.abs(K)) * (65 * U / 8)
    if dq is not None:
        sa = sa + np.einsum("pbhc,bhtc->pbht", np.asarray(dq, np.float64).reshape(nq, B, H, 64), np.abs(K)) / 8
    mx, lse, mean, empty = chunk_stats(s, V[None], T, chunks)
    ds, vmax = np.zeros(mx.shape), np.zeros(mx.shape)
    nk = np.zeros(chunks)
    for c, (lo, hi) in enumerate(chunk_bounds(T, chunks)):
        if hi > lo:
            ds[..., c] = sa[..., lo:hi].max(-1)
            vmax[..., c] = np.abs(V[:, :, lo:hi]).max(axis=(2, 3))[None]
            nk[c] = hi - lo
    return dict(mx=mx, lse=lse, mean=mean, empty=empty, ds=ds, vmax=vmax, nk=nk, out=merge_chunks(lse, mean), s=s, V=V,
                shape=(nq, B, H, chunks))


def combine_ref(records):
    """float64 combine of records [M][H][chunks][68] -> rows [M][64 H]"""
    r = np.asarray(records, np.float64)
    o, m, l = r[..., :64], r[..., 64], r[..., 65]
    w = np.exp(m - m.max(-1, keepdims=True))
    return ((w[..., None] * o).sum(-2) / (w * l).sum(-1)[..., None]).reshape(r.shape[0], -1)


# ----------------------------------------------------------------------------------------------------- checks ---
def check_self(res, qkv, kc, vc, pos0, npos, bf16, widen=False, margin=1.0, what=""):
    """res = (out, kcache, vcache) of a backend: caches bit for bit, out finite and within SELF_BAR (+ 2 ds max|v| where
    the case scales the scores) of float64"""
    out, kc_back, vc_back = res
    ref, kc2, vc2, ds, vmax = self_ref(qkv, kc, vc, pos0, npos, bf16)
    assert bits_equal(kc_back, kc2) and bits_equal(vc_back, vc2), (what, "cache")
    assert np.isfinite(out).all(), (what, "out not finite")
    rows, H = ds.shape
    err = np.abs(out - ref).reshape(rows, H, 64).max(-1)
    bar = SELF_BAR + (2 * ds * vmax if widen else 0.0)
    return _worst(err, bar, margin, what)


def check_records(ws, ref, widen=False, margin=1.0, what="", mask=None):
    """The three invariants of every record ws [nq * B][H][chunks][68] the prologue relies on, for the rows of `mask`
    [nq][B] (default all): o / l = the chunk's weighted mean of v (CROSS_BAR, + 2 ds max|v| where the case scales the
    scores), m + ln l = the chunk's logsumexp (ds + (80 + nk / 8) 2^-24 max(1, |lse|): ds on every score, then at most
    nk / 16 keys per 16-lane group with a multiply and an add each, a merge of at most 32 partials and the exp2 / log2
    roundings on l's longest chain), m = the chunk's maximum score to ds.  An empty chunk holds l = 0, o = 0 and a
    finite m."""
    nq, B, H, chunks = ref["shape"]
    sl = np.ones((nq, B), bool) if mask is None else mask
    w = np.asarray(ws, np.float64).reshape(nq, B, H, chunks, 68)[sl]
    assert np.isfinite(w[..., :66]).all(), (what, "records not finite")
    worst = 0.0
    for c in range(chunks):
        o, m, l = w[..., c, :64], w[..., c, 64], w[..., c, 65]
        if ref["empty"][c]:
            assert (l == 0).all() and (o == 0).all(), (what, "empty chunk", c)
            continue
        assert (l > 0).all(), (what, "l <= 0", c)
        ds, vmax, lse = ref["ds"][sl][..., c], ref["vmax"][sl][..., c], ref["lse"][sl][..., c]
        bar_o = CROSS_BAR + (2 * ds * vmax if widen else 0.0)
        worst = max(worst, _worst(np.abs(o / l[..., None] - ref["mean"][sl][..., c, :]).max(-1), bar_o, margin,
                                  (what, "o / l", c)))
        bar_lse = ds + (80 + ref["nk"][c] / 8) * U * np.maximum(1.0, np.abs(lse))
        worst = max(worst, _worst(np.abs(m + np.log(l) - lse), bar_lse, margin, (what, "m + ln l", c)))
        worst = max(worst, _worst(np.abs(m - ref["mx"][sl][..., c]), ds, margin, (what, "m", c)))
    return worst


def check_cross_out(out, ref, widen=False, margin=1.0, what="", mask=None):
    """the combined output [nq * B][d] against float64: CROSS_BAR (+ 2 ds max|v| over all chunks)"""
    nq, B, H, chunks = ref["shape"]
    assert np.isfinite(out).all(), (what, "out not finite")
    sl = np.ones((nq, B), bool) if mask is None else mask
    err = np.abs(np.asarray(out, np.float64).reshape(nq, B, H, 64) - ref["out"]).max(-1)[sl]
    bar = CROSS_BAR + (2 * (ref["ds"].max(-1) * ref["vmax"].max(-1))[sl] if widen else 0.0)
    return _worst(err, bar, margin, (what, "combined"))


def check_combine(Y, records, W, bias, R, bf16, guard, margin=1.0, what=""):
    """Y [M + n][d] of the combine tap: rows < M against float64 R + bias + combine(records) . W^T at GEMM_BAR of the
    largest output; the bf16 form on the bf16-rounded combined rows and weights plus the slack of an element within
    2^-20 |a| of a rounding boundary (the rule of ln_product_ref, tests/test_gpu_decoder_step.py); guard rows untouched."""
    M = records.shape[0]
    A = combine_ref(records)
    Wd = np.asarray(W, np.float64)
    slack = 0.0
    if bf16:
        Wd = bf16_round(W).astype(np.float64)
        win = 2.0 ** -20 * np.abs(A)
        lo = bf16_round((A - win).astype(np.float32)).astype(np.float64)
        hi = bf16_round((A + win).astype(np.float32)).astype(np.float64)
        slack = (hi - lo) @ np.abs(Wd).T
        A = bf16_round(A.astype(np.float32)).astype(np.float64)
    ref = np.asarray(R, np.float64) + np.asarray(bias, np.float64) + A @ Wd.T
    assert bits_equal(Y[M:], guard), (what, "guard rows written")
    assert np.isfinite(Y[:M]).all(), (what, "not finite")
    err = np.abs(Y[:M] - ref)
    return _worst(err, GEMM_BAR * np.abs(ref).max(), margin, what, slack)


# ------------------------------------------------------------------------------------------- float32 emulation ---
class Emu:
    """Plain float32 numpy emulation of the three launches behind the Engine's tap signatures."""

    def dbg_self_attention(self, qkv, kcache, vcache, pos, npos=1, bf16=False):
        rnd = bf16_round if bf16 else f32
        qkv = f32(qkv)
        B, cap, d = kcache.shape
        H = d // 64
        kc, vc = rnd(kcache).copy(), rnd(vcache).copy()
        q3 = qkv.reshape(npos, B, 3, d)
        kc[:, pos:pos + npos] = rnd(q3[:, :, 1]).transpose(1, 0, 2)
        vc[:, pos:pos + npos] = rnd(q3[:, :, 2]).transpose(1, 0, 2)
        out = np.zeros((npos, B, H, 64), np.float32)
        for p in range(npos):
            n = pos + p + 1
            K, V = kc[:, :n].reshape(B, n, H, 64), vc[:, :n].reshape(B, n, H, 64)
            q = q3[p, :, 0].reshape(B, H, 64) * np.float32(0.125)
            s = np.einsum("bhc,bnhc->bhn", q, K)
            e = np.exp(s - s.max(-1, keepdims=True))
            w = e / e.sum(-1, keepdims=True, dtype=np.float32)
            out[p] = np.einsum("bhn,bnhc->bhc", w, V)
        assert out.dtype == np.float32
        return out.reshape(npos * B, d), kc, vc

    @staticmethod
    def _queries(x, g, b, wq, bq):
        """fp32 two-pass LayerNorm and projection, scaled to log2 units as the kernel scales them"""
        x, g, b, wq, bq = (f32(a) for a in (x, g, b, wq, bq))
        d = np.float32(x.shape[1])
        mean = x.sum(1, keepdims=True, dtype=np.float32) / d
        t = x - mean
        rstd = np.float32(1.0) / np.sqrt((t * t).sum(1, keepdims=True, dtype=np.float32) / d + np.float32(1e-5))
        ln = t * rstd * g + b
        return (ln @ wq.T + bq) * np.float32(0.125 * LOG2E)

    def dbg_cross_attention_records(self, x, ln_g, ln_b, wq, bq, kc, vc, chunks=2, nq=1, bf16=False, row0=0, n_rows=None,
                                    guard=None):
        rnd = bf16_round if bf16 else f32
        B, H, T, _ = kc.shape
        n_rows = nq if n_rows is None else n_rows
        ws = np.full((nq * B, H, chunks, 68), 1e30, np.float32) if guard is None else f32(guard).copy()
        K, V = rnd(kc), rnd(vc)
        q = self._queries(f32(x)[row0 * B:(row0 + n_rows) * B], ln_g, ln_b, wq, bq).reshape(n_rows, B, H, 64)
        s = np.einsum("pbhc,bhtc->pbht", q, K)  # log2 units
        rec = ws[row0 * B:(row0 + n_rows) * B].reshape(n_rows, B, H, chunks, 68)
        for c, (lo, hi) in enumerate(chunk_bounds(T, chunks)):
            if hi <= lo:
                rec[..., c, :64], rec[..., c, 64], rec[..., c, 65] = 0.0, EMPTY_M, 0.0
                continue
            m = s[..., lo:hi].max(-1)
            p = np.exp2(s[..., lo:hi] - m[..., None])
            assert p.dtype == np.float32
            rec[..., c, :64] = np.einsum("pbht,bhtc->pbhc", p, V[:, :, lo:hi])
            rec[..., c, 64] = m * np.float32(1.0 / LOG2E)
            rec[..., c, 65] = p.sum(-1, dtype=np.float32)
        return ws

    @staticmethod
    def _combine(records):
        r = f32(records)
        o, m, l = r[..., :64], r[..., 64], r[..., 65]
        w = np.exp(m - m.max(-1, keepdims=True))
        ls = (w * l).sum(-1, dtype=np.float32)
        a = (w[..., None] * o).sum(-2, dtype=np.float32) * (np.float32(1.0) / ls)[..., None]
        assert a.dtype == np.float32
        return a.reshape(r.shape[0], -1)

    def dbg_cross_combine(self, records, W, bias, R, B, bf16=False, guard=None):
        A, W = self._combine(records), f32(W)
        if bf16:
            A, W = bf16_round(A), bf16_round(W)
        Y = f32(R) + f32(bias) + A @ W.T
        return Y if guard is None else np.concatenate([Y, f32(guard)])

    def dbg_cross_attention(self, x, ln_g, ln_b, wq, bq, kc, vc, chunks=2, nq=1, bf16=False):
        return self._combine(self.dbg_cross_attention_records(x, ln_g, ln_b, wq, bq, kc, vc, chunks, nq, bf16))


# ------------------------------------------------------------------------------------------------ case inputs ---
def cross_inputs(rng, B, H, T, nq, bf16, wq_scale=1.0):
    """ordinary unit-variance inputs of the cross-attention taps (the caches bf16-rounded for the bf16 form)"""
    d = H * 64
    rnd = bf16_round if bf16 else f32
    x = (rng.standard_normal((nq * B, d)) * 2 + 0.3).astype(np.float32)
    g = (1 + 0.2 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    wq = (rng.standard_normal((d, d)) / np.sqrt(d) * wq_scale).astype(np.float32)
    bq = (0.1 * rng.standard_normal(d)).astype(np.float32)
    kc = rnd(rng.standard_normal((B, H, T, 64)).astype(np.float32))
    vc = rnd(rng.standard_normal((B, H, T, 64)).astype(np.float32))
    return x, g, b, wq, bq, kc, vc


def _self_inputs(rng, B, H, cap, pos0, npos, stale=0.0):
    """qkv and caches whose rows < pos0 are filled; every row at or behind pos0 holds `stale`"""
    d = 64 * H
    kc, vc = np.full((B, cap, d), stale, np.float32), np.full((B, cap, d), stale, np.float32)
    kc[:, :pos0] = rng.standard_normal((B, pos0, d))
    vc[:, :pos0] = rng.standard_normal((B, pos0, d))
    return rng.standard_normal((npos * B, 3 * d)).astype(np.float32), kc, vc


def _run_self(eng, qkv, kc, vc, pos0, npos, bf16, margin, what, widen=False):
    res = eng.dbg_self_attention(qkv, kc, vc, pos0, npos, bf16=bf16)
    return check_self(res, qkv, kc, vc, pos0, npos, bf16, widen, margin, what), res


# ------------------------------------------------------------------------------- A. self_attention_step cases ---
def a1_every_position(eng, H, bf16, margin=1.0):
    """positions 0..31, one per launch, chained through the returned cache"""
    rng = np.random.default_rng(100 + H)
    B, cap, d = 3, 32, 64 * H
    kc, vc = np.zeros((B, cap, d), np.float32), np.zeros((B, cap, d), np.float32)
    worst = 0.0
    for pos in range(32):
        qkv = rng.standard_normal((B, 3 * d)).astype(np.float32)
        r, (_, kc, vc) = _run_self(eng, qkv, kc, vc, pos, 1, bf16, margin, ("A1", H, pos))
        worst = max(worst, r)
    return worst


A2_GROUPS = [(0, 1, 5, 6), (0, 2, 5, 6), (0, 3, 5, 6), (0, 4, 5, 6), (1, 4, 5, 6), (27, 4, 5, 6), (28, 4, 5, 6), (29, 3, 5, 6),
             (31, 1, 5, 6), (0, 32, 2, 2)]


def a2_prompt_group(eng, pos0, npos, B, H, bf16, margin=1.0):
    rng = np.random.default_rng(200 + pos0 * 40 + npos)
    qkv, kc, vc = _self_inputs(rng, B, H, 32, pos0, npos)
    return _run_self(eng, qkv, kc, vc, pos0, npos, bf16, margin, ("A2", pos0, npos))[0]


A3_WIDTHS = [(1, 17, 1), (32, 17, 1), (64, 17, 1), (128, 17, 1), (32, 13, 4)]


def a3_chain_width(eng, B, pos0, npos, bf16, margin=1.0):
    """every row of a chain-wide launch (rows p * B + b)"""
    rng = np.random.default_rng(300 + B + npos)
    qkv, kc, vc = _self_inputs(rng, B, 6, 32, pos0, npos)
    return _run_self(eng, qkv, kc, vc, pos0, npos, bf16, margin, ("A3", B, npos))[0]


A4_CAPS = (32, 33, 224, 448)


def a4_stride_and_stale_rows(eng, cap, bf16, margin=1.0):
    """the b * cap * d stride of a longer cache; every row at or behind pos0 + npos holds NaN (at pos0 = 0 row 0 too, which
    the kernel loads and must not use) and comes back bit-identical (check_self compares the caches' bits)"""
    rng = np.random.default_rng(400 + cap)
    worst = 0.0
    for pos0, npos in ((0, 1), (0, 4), (5, 1), (17, 3), (28, 4), (31, 1)):
        qkv, kc, vc = _self_inputs(rng, 3, 2, cap, pos0, npos, stale=np.nan)
        worst = max(worst, _run_self(eng, qkv, kc, vc, pos0, npos, bf16, margin, ("A4", cap, pos0, npos))[0])
    return worst


def a5_bit_identity(eng, bf16, margin=1.0):
    """a clip alone and as clip 2 of 3 and of 128: the same bits in out and in its cache rows"""
    worst = 0.0
    for pos0, npos in ((17, 1), (0, 4)):
        rng = np.random.default_rng(500 + pos0)
        H, d = 6, 384
        qkv, kc, vc = _self_inputs(rng, 128, H, 32, pos0, npos)
        q3 = qkv.reshape(npos, 128, 3 * d)
        r, (o1, k1, v1) = _run_self(eng, q3[:, 1].copy(), kc[1:2], vc[1:2], pos0, npos, bf16, margin, ("A5 alone", pos0))
        worst = max(worst, r)
        for B in (3, 128):
            r, (o, k, v) = _run_self(eng, q3[:, :B].reshape(npos * B, 3 * d).copy(), kc[:B], vc[:B], pos0, npos, bf16, margin,
                                     ("A5", B, pos0))
            worst = max(worst, r)
            assert bits_equal(o.reshape(npos, B, d)[:, 1], o1.reshape(npos, d)), ("A5 out", B, pos0)
            assert bits_equal(k[1], k1[0]) and bits_equal(v[1], v1[0]), ("A5 cache", B, pos0)
    return worst


A6_REGIMES = ("dominant", "zero_q", "shift", "spread")


def _regime_keys(rng, regime, q, n, dom):
    """keys [..., n][64] for queries q [...][64] under a softmax regime; dom [...] = index of the dominating key.  Scores
    are q . k / 8."""
    lead = q.shape[:-1]
    k = rng.standard_normal(lead + (n, 64))
    qq = (q * q).sum(-1)
    if regime == "dominant":  # one key at score 250, the others O(1): a margin above 200
        idx = np.indices(lead)
        k[tuple(idx) + (dom,)] = q * (8 * 250.0 / qq)[..., None]
    elif regime == "shift":   # a common component: 512 * 512 / 8 = 32768 on every score, exact in fp32 and bf16
        k[..., 0] = 512.0
    elif regime == "spread":  # scores spread over +-50, in a shuffled order
        t = rng.permuted(np.broadcast_to(np.linspace(-50.0, 50.0, n), lead + (n,)), axis=-1)
        k = 0.1 * k + q[..., None, :] * (8 * t / qq[..., None])[..., None]
    return k


def a6_softmax_regime(eng, regime, bf16, margin=1.0):
    """per head at H = 6, pos = 31; the dominating key sits at key 0, 15, 30 or the new position (31), by head and clip"""
    rng = np.random.default_rng(600 + A6_REGIMES.index(regime))
    B, H, cap, pos, d = 3, 6, 32, 31, 384
    q = rng.standard_normal((B, H, 64))
    if regime == "zero_q":
        q[:] = 0.0
    if regime == "shift":
        q[..., 0] = 512.0
    dom = np.array([0, 15, 30, 31])[(np.arange(B)[:, None] + np.arange(H)[None]) % 4]
    k = _regime_keys(rng, regime, q, 32, dom)                      # [B][H][32][64]
    v = rng.standard_normal((B, H, 32, 64))
    rnd = bf16_round if bf16 else f32
    kc = rnd(k.transpose(0, 2, 1, 3).reshape(B, 32, d))
    vc = rnd(v.transpose(0, 2, 1, 3).reshape(B, 32, d))
    qkv = np.concatenate([q.reshape(B, d), kc[:, pos], vc[:, pos]], axis=1).astype(np.float32)
    kc0, vc0 = kc.copy(), vc.copy()
    kc0[:, pos], vc0[:, pos] = 0.0, 0.0
    widen = regime in ("shift", "spread")
    r, (out, _, _) = _run_self(eng, qkv, kc0, vc0, pos, 1, bf16, margin, ("A6", regime), widen)
    o = out.reshape(B, H, 64)
    vv = vc.reshape(B, 32, H, 64)
    if regime == "dominant":  # the output IS that key's v
        want = np.take_along_axis(vv.transpose(0, 2, 1, 3), dom[..., None, None], axis=2)[:, :, 0]
        assert np.abs(o - want).max() <= margin * SELF_BAR, ("A6 dominant", np.abs(o - want).max())
    if regime == "zero_q":    # the output is the mean of v
        want = vv.astype(np.float64).mean(1)
        assert np.abs(o - want).max() <= margin * SELF_BAR, ("A6 zero_q", np.abs(o - want).max())
    return r


# ------------------------------------------------------------------------------ B. cross_attention_step cases ---
def _run_cross(eng, inp, chunks, nq, bf16, margin, what, widen=False, dq=None, combined=True):
    ref = cross_ref(*inp, chunks, nq, bf16, dq)
    ws = eng.dbg_cross_attention_records(*inp, chunks, nq, bf16=bf16)
    r = check_records(ws, ref, widen, margin, what)
    if combined:
        r = max(r, check_cross_out(eng.dbg_cross_attention(*inp, chunks, nq, bf16=bf16), ref, widen, margin, what))
    return r, ws, ref


def b1_instantiation(eng, nq, H, bf16, margin=1.0):
    rng = np.random.default_rng(1000 + 10 * nq + H)
    return _run_cross(eng, cross_inputs(rng, 2, H, 70, nq, bf16), 2, nq, bf16, margin, ("B1", nq, H))[0]


def b2_geometry(eng, bf16, margin=1.0):
    """T on the load-round edges (16 and 64 keys in fp32, 32 and 128 in bf16) x chunks, empty chunks included"""
    worst = 0.0
    for T, chunks in GEOMETRY:
        rng = np.random.default_rng(2000 + 10 * T + chunks)
        worst = max(worst, _run_cross(eng, cross_inputs(rng, 2, 2, T, 1, bf16), chunks, 1, bf16, margin, ("B2", T, chunks))[0])
    return worst


def b2_full_length(eng, bf16, margin=1.0):
    rng = np.random.default_rng(2999)
    return _run_cross(eng, cross_inputs(rng, 4, 6, 1500, 4, bf16), 8, 4, bf16, margin, ("B2", 1500))[0]


def b3_masked_past_keys(eng, bf16, margin=1.0):
    """The last key of every chunk carries half of the chunk's softmax weight and v = 4 in every component (larger values
    would leave the unit-variance bar behind fp32's own rounding): a past key of the last load round (a re-read of that
    row) counted once would raise its weight to 2 / 3 and move o / l by about 4 / 6.  nk = 35 and nk = 200 end in a partial round
    in both forms (rounds of 64 keys in fp32, 128 in bf16)."""
    worst = 0.0
    for T, chunks in ((70, 2), (200, 1), (129, 1)):
        rng = np.random.default_rng(3000 + T)
        x, g, b, wq, bq, kc, vc = cross_inputs(rng, 2, 6, T, 1, bf16)
        q = query_ref(x, g, b, wq, bq).reshape(2, 6, 64)
        kc, vc = kc.astype(np.float64), vc.astype(np.float64)
        for lo, hi in chunk_bounds(T, chunks):
            s = np.einsum("bhc,bhtc->bht", q, kc[:, :, lo:hi - 1]) / 8
            lse = s.max(-1) + np.log(np.exp(s - s.max(-1, keepdims=True)).sum(-1))
            kc[:, :, hi - 1] = q * (8 * lse / (q * q).sum(-1))[..., None]  # score = the logsumexp of the others
            vc[:, :, hi - 1] = 4.0
        rnd = bf16_round if bf16 else f32
        inp = (x, g, b, wq, bq, rnd(kc), rnd(vc))
        r, ws, ref = _run_cross(eng, inp, chunks, 1, bf16, margin, ("B3", T))
        w_last = np.exp(ref["s"][0][..., [hi - 1 for _, hi in chunk_bounds(T, chunks)]] - ref["lse"][0])
        assert (np.abs(w_last - 0.5) < 0.05).all(), ("B3: the planted key does not carry half the weight", w_last)
        worst = max(worst, r)
    return worst


def b4_layernorm_inside(eng, bf16, margin=1.0):
    """rows 1e3 + N(0, 1) and constant rows (3.0, -0.75, 0.0) among ordinary ones, H = 6, nq = 4.  Ordinary and constant
    rows (LN = ln_b exactly, q = Wq ln_b + bq) at the ordinary bars.  Offset rows: the LayerNorm of such a row is held
    to 1e-2 of its largest |LN| (test_ln_row_statistics_edges), so |dq_c| <= 1e-2 max|LN| sum_k |Wq_ck|, which enters ds
    through |k| and the output bar as 2 ds max|v|; Wq is N(0, 1 / d) / 64 to keep that bar below the outputs' spread."""
    rng = np.random.default_rng(4000)
    B, H, T, nq, chunks = 4, 6, 70, 4, 2
    x, g, b, wq, bq, kc, vc = cross_inputs(rng, B, H, T, nq, bf16, wq_scale=1.0 / 64)
    offset, const = [1, 6, 11, 12], {2: 3.0, 7: -0.75, 13: 0.0}
    x[offset] = (1e3 + rng.standard_normal((len(offset), H * 64))).astype(np.float32)
    for r, val in const.items():
        x[r] = val
    dq = np.zeros((nq * B, H * 64))
    dq[offset] = 1e-2 * np.abs(ln64(x, g, b)[offset]).max(1, keepdims=True) * np.abs(wq.astype(np.float64)).sum(1)[None]
    inp = (x, g, b, wq, bq, kc, vc)
    ref_plain, ref_off = cross_ref(*inp, chunks, nq, bf16), cross_ref(*inp, chunks, nq, bf16, dq)
    ws = eng.dbg_cross_attention_records(*inp, chunks, nq, bf16=bf16)
    out = eng.dbg_cross_attention(*inp, chunks, nq, bf16=bf16)
    is_off = np.zeros(nq * B, bool)
    is_off[offset] = True
    off = is_off.reshape(nq, B)
    return max(check_records(ws, ref_plain, False, margin, "B4 ordinary", ~off),
               check_cross_out(out, ref_plain, False, margin, "B4 ordinary", ~off),
               check_records(ws, ref_off, True, margin, "B4 offset", off),
               check_cross_out(out, ref_off, True, margin, "B4 offset", off))


B5_CASES = [("dominant", 300, (5,)), ("dominant", 300, (140,)), ("dominant", 300, (149,)), ("dominant", 40, (10,)),
            ("zero_q", 300, ()), ("shift", 300, ()), ("spread", 300, ())]


def b5_softmax_regime(eng, regime, T, at, bf16, margin=1.0):
    """Wq = 0, so q = bq for every row.  chunks = 2.  The dominating key of each chunk (score 250) sits at chunk index `at`
    : 5 = the first load round, 140 = a later round in both
    forms, 149 = the chunk's last key (nk = 150); at nk = 20, key 10 is the only key of its 16- and of its 8-lane group."""
    rng = np.random.default_rng(5000 + T + sum(at))
    B, H, nq, chunks, d = 2, 6, 2, 2, 384
    x, g, b, wq, bq, kc, vc = cross_inputs(rng, B, H, T, nq, bf16)
    wq[:] = 0.0
    bq = rng.standard_normal(d).astype(np.float32)
    if regime == "zero_q":
        bq[:] = 0.0
    if regime == "shift":
        bq[0::64] = 512.0
    q = np.broadcast_to(bq.astype(np.float64).reshape(1, H, 64), (B, H, 64))
    k = np.zeros((B, H, T, 64))
    for lo, hi in chunk_bounds(T, chunks):
        dom = np.full((B, H), at[0] if at else 0)
        k[:, :, lo:hi] = _regime_keys(rng, regime, q, hi - lo, dom)
    rnd = bf16_round if bf16 else f32
    inp = (x, g, b, wq, bq, rnd(k), vc)
    r, ws, ref = _run_cross(eng, inp, chunks, nq, bf16, margin, ("B5", regime, T, at), widen=regime in ("shift", "spread"))
    w5 = np.asarray(ws, np.float64).reshape(nq, B, H, chunks, 68)
    mean = w5[..., :64] / w5[..., 65:66]
    V = ref["V"]
    for c, (lo, hi) in enumerate(chunk_bounds(T, chunks)):
        if regime == "dominant":  # o / l IS the dominating key's v
            assert np.abs(mean[..., c, :] - V[None, :, :, lo + at[0]]).max() <= margin * CROSS_BAR, ("B5 dominant", c)
        if regime == "zero_q":    # o / l is the chunk's mean of v
            assert np.abs(mean[..., c, :] - V[None, :, :, lo:hi].mean(3)).max() <= margin * CROSS_BAR, ("B5 zero_q", c)
    return r


def b6_bit_identity_and_grouping(eng, bf16, margin=1.0):
    """Returns (worst err / bar, the largest difference between one nq = 4 launch and four nq = 1 launches)."""
    rng = np.random.default_rng(6000)
    B, H, T, nq, chunks = 32, 6, 70, 4, 2
    inp = cross_inputs(rng, B, H, T, nq, bf16)
    x, g, b, wq, bq, kc, vc = inp
    d = H * 64
    ref = cross_ref(*inp, chunks, nq, bf16)
    ws = eng.dbg_cross_attention_records(*inp, chunks, nq, bf16=bf16)
    worst = check_records(ws, ref, False, margin, "B6 batch")
    # clip 5 alone: the same bits
    x1 = x.reshape(nq, B, d)[:, 5].copy()
    ws1 = eng.dbg_cross_attention_records(x1, g, b, wq, bq, kc[5:6], vc[5:6], chunks, nq, bf16=bf16)
    assert bits_equal(f32(ws).reshape(nq, B, H, chunks, 68)[:, 5, :, :, :66], f32(ws1).reshape(nq, H, chunks, 68)[..., :66]), "B6 alone"
    # four nq = 1 launches into one guarded buffer; each leaves every other record's guard pattern untouched
    guard = rng.standard_normal((nq * B, H, chunks, 68)).astype(np.float32)
    split = guard.copy()
    for p in range(nq):
        one = eng.dbg_cross_attention_records(*inp, chunks, nq, bf16=bf16, row0=p, n_rows=1, guard=guard)
        rows = slice(p * B, (p + 1) * B)
        mask = np.ones(nq * B, bool)
        mask[rows] = False
        assert bits_equal(one[mask], guard[mask]), ("B6 guard", p)
        split[rows] = one[rows]
    worst = max(worst, check_records(split, ref, False, margin, "B6 four launches"))
    # positions 1 .. 3 of the four, as the engine's position loop addresses a later group
    part = eng.dbg_cross_attention_records(*inp, chunks, nq, bf16=bf16, row0=1, n_rows=3, guard=guard)
    assert bits_equal(part[:B], guard[:B]), "B6 guard in front"
    later = np.ones((nq, B), bool)
    later[0] = False
    worst = max(worst, check_records(part, ref, False, margin, "B6 sub-range", later))
    diff = float(np.abs(f32(ws)[..., :66].astype(np.float64) - split[..., :66]).max())
    return worst, diff


# ------------------------------------------------------------------------------------ C. the combine prologue ---
def random_records(rng, M, H, chunks):
    """records with m spread over +-30, l in [0.5, 2), o ~ N(0, 1) l"""
    rec = rng.standard_normal((M, H, chunks, 68)).astype(np.float32)
    rec[..., 64] = rng.uniform(-30, 30, (M, H, chunks))
    rec[..., 65] = rng.uniform(0.5, 2.0, (M, H, chunks))
    rec[..., :64] *= rec[..., 65:66]
    return rec


def combine_operands(rng, M, H):
    d = 64 * H
    W = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    return W, rng.standard_normal(d).astype(np.float32), rng.standard_normal((M, d)).astype(np.float32), \
        rng.standard_normal((3, d)).astype(np.float32)


def c1_shapes(eng, H, bf16, margin=1.0):
    worst = 0.0
    for chunks in (1, 2, 4, 8):
        for M, B in COMBINE_ROWS:
            rng = np.random.default_rng(7000 + 100 * chunks + M + H)
            rec = random_records(rng, M, H, chunks)
            W, bias, R, guard = combine_operands(rng, M, H)
            Y = eng.dbg_cross_combine(rec, W, bias, R, B, bf16=bf16, guard=guard)
            worst = max(worst, check_combine(Y, rec, W, bias, R, bf16, guard, margin, ("C1", chunks, M, H)))
    return worst


def c1_last_tile_of_one_row(eng, H, bf16, margin=1.0):
    """M = 33 and 97 again, six times each behind allocations that held huge values: the last 32-row tile has ONE row and
    its other 31 lanes are clamped onto it, so every lane of the tile loads one cached record and the loads in front of
    the tile's first MFMA have landed when it issues.  That is the timing at which the bf16 form took a stale A
    operand; every repetition carries the bits of the first."""
    worst = 0.0
    for chunks in (1, 2, 4, 8):
        for M, B in ((33, 11), (97, 97)):
            rng = np.random.default_rng(7000 + 100 * chunks + M + H)
            rec = random_records(rng, M, H, chunks)
            W, bias, R, guard = combine_operands(rng, M, H)
            first = None
            for rep in range(6):
                huge = np.float32([3e34, -7e33, 1e30, 5e36, -2e34, 1e25][rep])
                eng.dbg_cross_combine(np.abs(rec) * huge, W, bias, R * huge, B, bf16=bf16, guard=guard * huge)
                Y = eng.dbg_cross_combine(rec, W, bias, R, B, bf16=bf16, guard=guard)
                worst = max(worst, check_combine(Y, rec, W, bias, R, bf16, guard, margin, ("C1 one-row tile", chunks, M, H, rep)))
                first = Y if first is None else first
                assert bits_equal(Y, first), ("C1 one-row tile: not repeatable", chunks, M, H, rep)
    return worst


def c2_extremes(eng, chunks, bf16, margin=1.0):
    """rows 0..6 of M = 33 carry the extremes, the rest are ordinary"""
    rng = np.random.default_rng(7500 + chunks)
    M, B, H = 33, 11, 2
    rec = random_records(rng, M, H, chunks)
    empty = np.zeros(68, np.float32)
    empty[64] = EMPTY_M
    rec[0, :, 1] = empty                      # one record exactly as the kernel writes an empty chunk
    rec[1] = empty                            # all chunks empty but one
    rec[1, :, 2] = random_records(rng, 1, H, 1)[0, :, 0]
    rec[2, :, :, 64] = -100.0                 # maxima 200 apart: the small ones underflow to zero weight
    rec[2, :, 3, 64] = 100.0
    rec[3, :, :, 64] = 1.25                   # equal maxima
    rec[4, :, :, 64] = 80.0 + rng.uniform(-1, 1, (H, chunks))   # only differences may matter
    rec[5, :, :, 64] = -80.0 + rng.uniform(-1, 1, (H, chunks))
    rec[6] = 1e30                             # another row's records: a wrong row or head index shows in rows 5 and 7
    W, bias, R, guard = combine_operands(rng, M, H)
    Y = eng.dbg_cross_combine(rec, W, bias, R, B, bf16=bf16, guard=guard)
    return check_combine(Y, rec, W, bias, R, bf16, guard, margin, ("C2", chunks))


def c3_kernel_to_prologue(eng, bf16):
    """real records through the combine tap with W = identity, no bias, no residual: the bits of the path tap (whose
    out-projection runs in the fp32-plane form in both storage modes)"""
    for H, T, chunks, nq, B in ((2, 9, 8, 1, 2), (6, 70, 2, 4, 2), (8, 129, 4, 3, 5), (6, 1500, 8, 4, 4)):
        rng = np.random.default_rng(8000 + T)
        inp = cross_inputs(rng, B, H, T, nq, bf16)
        d = 64 * H
        ws = eng.dbg_cross_attention_records(*inp, chunks, nq, bf16=bf16)
        out = eng.dbg_cross_attention(*inp, chunks, nq, bf16=bf16)
        Y = eng.dbg_cross_combine(ws, np.eye(d, dtype=np.float32), np.zeros(d, np.float32), np.zeros((nq * B, d), np.float32), B)
        assert bits_equal(Y, out), ("C3", H, T, chunks)
