"""Cases, float64 reference, bars and a float32 emulation for the encoder GEMMs that write the NEXT LayerNorm from their own
epilogue: planes_epilogue<..., LN = true> of k_gemm_planes.hip (fp16 planes, N = 384, tiles 192 x 384 and
256 x 384) and bf16_epilogue<..., LN> of k_gemm_bf16.hip (tiles 192 x 128, 192 x 384, 128 x 512), through the tap
wt_dbg_gemm_ln_fused (Engine.dbg_gemm_ln_fused).

Layers, as in decoder_attn_ref.py:
  * the case lists (PLANE_TABLE, plane_cases, conv2_case, bf16_cases, edge_case, flag shapes) and plane_plan_model /
    bf16_plan_model, the launchers' tile choice restated in Python, which says which kernel a case must reach;
  * reference(): float64, gather rows - contract - epilogue - LayerNorm with eps 1e-5 (the bf16 family on bf16-rounded
    operands, as its sibling tests);
  * Emu: a float32 numpy emulation of the kernels' arithmetic behind the tap's signature: fp32 accumulation over the 32-deep MFMA steps, then two-pass
    statistics over the partial sums of the WN wavefront columns of a block row (4 x 96 columns; bf16: 4 x 128, 4 x 96 or
    2 x 64), each summed per lane (NI x 4 values) and over 8 lanes by a butterfly, as the kernels do.  Emu(defect=...)
    is deliberately wrong in one of five ways (DEFECTS);
  * check() / run_case() / flag_checks(): every assertion, as functions of a backend (an Engine, or Emu) and a margin.
    tests/test_gpu_gemm_ln_fused.py runs them on the GPU with margin 1, tests/test_gemm_ln_reference.py on Emu with
    margin 1/4 (a correct fp32 kernel can meet the bars) and on every defective Emu (which must fail).

Bars.  C: 3e-6 relative to the largest output (FP32_TOL of test_gpu_encoder_handover.py).  ln_y32 against the float64
LayerNorm of the RETURNED C: 5e-6 on ordinary rows, the bar of test_layernorm_planes: the fused code is given the same x and
computes the same function.  ln_y32 against the whole float64 chain: 1e-5 (test_plane_gemm_with_fused_layernorm), ordinary
rows only (an edge row's C carries an error of 2^-24 |mean|, which its LayerNorm magnifies by rstd: no fixed bar applies).
Edge rows, against the LayerNorm of the returned C, per element:
    EDGE_C * 2^-24 * (|mean| + max |x - mean|) * rstd * max |g|  +  2^-23 |y|
(the rounding of the sums and of x - mean is relative to the row's magnitude and reaches y times rstd |g|; the last
operations round y itself).  EDGE_C is the smallest power of two at which Emu stays under a quarter of the bound on every
edge row; test_gemm_ln_reference.py derives it again and compares.  Planes: bit for bit the fp16 split of
float32(ln_y32 * ln_scale), or the round-to-nearest-even bf16 of ln_y32.  Guards: every word as given."""
from types import SimpleNamespace

import numpy as np
from scipy.special import erf

BIAS, GELU, RESIDUAL, POS = 1, 2, 4, 8
EPI_RESIDUAL, EPI_CONV = BIAS | RESIDUAL, BIAS | GELU | POS
CONTIGUOUS = 1 << 30
GUARD = 256            # rows behind every output: one whole tile of the tallest kernel
U = 2.0 ** -24
C_BAR = 3e-6
LN_OF_C_BAR = 5e-6
CHAIN_BAR = 1e-5
EDGE_C = 8            # derived by derive_edge_c(); test_gemm_ln_reference.py holds it to that
LN_SCALES = (1.0, 64.0, 1024.0)
DEFECTS = ("one_pass_variance", "rows_past_m", "row_map_rotated", "flag_first_wave_row", "scale_on_lo_only")
TILE_NAMES = ("192x128", "192x384", "256x384")

# (tile the launcher must choose, M, n_cu): the edges of the issue's table, derived from the cost model of plane_gemm_plan
PLANE_TABLE = [
    (1, 1, 1),      # one row
    (1, 192, 1),    # exactly one tile
    (1, 193, 2),    # last tile of one row
    (1, 289, 1),    # second wavefront row of the last tile holds one row
    (1, 384, 2),    # two whole tiles
    (2, 193, 1),    # 193 of 256 rows
    (2, 256, 1),    # exactly one tile
    (2, 385, 1),    # second wavefront row of the last tile holds one row
    (2, 512, 1),    # two whole tiles
]
PLANE_KS = (32, 96, 384)                     # one k-tile, an odd count, d_model
EPILOGUES = ((EPI_RESIDUAL, 0), (EPI_CONV, 32), (EPI_CONV, 100))   # (epi, pos_period): 32 is the contract's minimum
# bf16 family: N -> (rows of the whole-row tile, M = 1, one tile plus one row, two whole tiles)
BF16_ROWS = {128: (1, 193, 384), 384: (1, 193, 384), 512: (1, 129, 256)}
BF16_KS = (64, 192)
# (family, N, M, n_cu) of the flag tests: row M - 1 is alone in the SECOND wavefront row of a ragged last tile
FLAG_SHAPES = [(0, 384, 289, 1), (0, 384, 385, 1), (1, 384, 289, 0), (1, 128, 289, 0), (1, 512, 193, 0)]
# (family, N, M, n_cu): the last tile holds one row.  The 256 x 384 tile is the exception: within 512 rows the cost model
# gives it no such shape (M = 257 goes to the 192-row tile at every n_cu), so it runs with one row in the second
# wavefront row of its last tile
REPEAT_SHAPES = [(0, 384, 193, 2), (0, 384, 385, 1), (1, 128, 193, 0), (1, 384, 193, 0), (1, 512, 129, 0)]


# ------------------------------------------------------------------------------------------------ the tile choice ---
def plane_plan_model(M, N, K, epi, planes_out, ln, n_cu, mode=2):
    """plane_gemm_plan of k_gemm_planes.hip restated: (tile, schedule, fused).  cost = rows x 128-column units x rounds of
    the CUs; narrow 192 x 128: x 1.1, tall 256 x 384: x 1.08."""
    cu = n_cu if n_cu > 0 else 256
    rounds = lambda tiles: (tiles + cu - 1) // cu
    rt192, rt256 = (M + 191) // 192, (M + 255) // 256
    wide_ok = N % 384 == 0
    c_wide = 192.0 * 3 * rounds(rt192 * (N // 384)) if wide_ok else 1e30
    c_tall = 256.0 * 3 * 1.08 * rounds(rt256 * (N // 384)) if wide_ok else 1e30
    c_narrow = 192.0 * 1.1 * rounds(rt192 * (N // 128))
    tile = (2 if c_tall < c_wide else 1) if c_wide <= c_narrow else (2 if c_tall < c_narrow else 0)
    fused = bool(ln) and not planes_out and epi in (EPI_RESIDUAL, EPI_CONV) and N == 384 and tile != 0
    schedule = 0
    if tile == 1:
        blocks, kt = rt192 * (N // 384), K // 32
        persist = (planes_out and not fused and (epi & ~(BIAS | GELU)) == 0 and mode == 2 and cu % 8 == 0 and blocks >= 2 * cu
                   and kt % 2 == 0 and kt >= 4)
        schedule = 3 if persist else 2 if mode in (2, 4) else 1 if mode == 1 else 0
    return tile, schedule, fused


def bf16_plan_model(M, N, epi, bf16_out, ln, c_rpb=CONTIGUOUS, ldc=None):
    """bf16_gemm_plan of k_gemm_bf16.hip restated: (bn, bm, whole_row)."""
    ldc = N if ldc is None else ldc
    if ln and not bf16_out and ldc == N and c_rpb >= M and N in (128, 384, 512) and epi in (EPI_RESIDUAL, EPI_CONV):
        return N, (128 if N == 512 else 192), True
    return (384 if N % 384 == 0 else 256 if N % 256 == 0 else 128), 192, False


def geometry(family, M, N, K, epi, n_cu):
    """(rows of the block tile, wavefront columns that share a row's sums, name) of the fused kernel the case reaches"""
    if family == 0:
        tile, _, fused = plane_plan_model(M, N, K, epi, False, True, n_cu)
        assert fused, ("the plane GEMM would not fuse here", M, N, n_cu, TILE_NAMES[tile])
        return (192 if tile == 1 else 256), 4, TILE_NAMES[tile]
    bn, bm, whole = bf16_plan_model(M, N, epi, False, True)
    assert whole, ("the bf16 GEMM would not fuse here", M, N)
    return bm, (2 if N == 128 else 4), f"bf16 {bm}x{bn}"


# ---------------------------------------------------------------------------------------------------------- helpers ---
def f32(x):
    return np.ascontiguousarray(x, np.float32)


def gelu(x):
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def bf16_bits(x):
    """round to nearest even; a NaN stays a NaN"""
    u = f32(x).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_round(x):
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def exact_split(a):
    """numpy's fp16 split of float32 a: hi = fp16(a), lo = fp16(a - hi), both round to nearest even (a - hi is exact)"""
    a = f32(a)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = a.astype(np.float16)
        return hi, (a - hi.astype(np.float32)).astype(np.float16)


def gather_rows(a_flat, M, K, a_rpb, a_bs, lda):
    m = np.arange(M)
    start = (m // a_rpb) * a_bs + (m % a_rpb) * lda
    return a_flat[start[:, None] + np.arange(K)[None, :]]


def ln64(x, g, b):
    x = np.asarray(x, np.float64)
    return (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


# ------------------------------------------------------------------------------------------------------------ cases ---
def make_case(family, N, M, K, epi, n_cu=0, pos_period=0, ln_scale=64.0, form="dense", seed=0, fusable=True):
    """Operands as the sibling tests draw them: A standard normal, W standard normal / sqrt(K), bias and pos standard
    normal, the residual N(0.7, 3), gain 1 + 0.3 N(0, 1), shift N(0, 1).  form "conv2": rows overlapping with stride 2 as
    conv2 reads them (a_rpb = T = M / 3 clips, a_bs = (2 T + 2) d_in, lda = 2 d_in, K = 3 d_in)."""
    rng = np.random.default_rng(1000 * (seed + 1) + 97 * family + 31 * epi + M + N + K + pos_period)
    if form == "conv2":
        T, d_in = M // 3, K // 3
        a_rpb, a_bs, lda = T, (2 * T + 2) * d_in, 2 * d_in
        a_len = 3 * a_bs
    else:
        a_rpb, a_bs, lda, a_len = CONTIGUOUS, 0, K, M * K
    bm, wn, kernel = geometry(family, M, N, K, epi, n_cu) if fusable else (192, 0, "not fused")
    return SimpleNamespace(
        name=f"{'bf16' if family else 'planes'}-{form}-M{M}-N{N}-K{K}-epi{epi}-p{pos_period}-cu{n_cu}-s{ln_scale:g}",
        family=family, N=N, M=M, K=K, epi=epi, n_cu=n_cu, ln_scale=float(ln_scale), bm=bm, wn=wn, kernel=kernel,
        A=rng.standard_normal(a_len).astype(np.float32), a_rpb=a_rpb, a_bs=a_bs, lda=lda,
        W=(rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), bias=rng.standard_normal(N).astype(np.float32),
        R=(rng.standard_normal((M, N)) * 3 + 0.7).astype(np.float32) if epi & RESIDUAL else None,
        pos=rng.standard_normal((pos_period, N)).astype(np.float32) if epi & POS else None,
        g=(1.0 + 0.1 * rng.standard_normal(N)).astype(np.float32), b=rng.standard_normal(N).astype(np.float32),
        edge={}, fills=fills(M, N, seed + M + K))


def fills(M, N, seed):
    """what the outputs hold before the launch (ln_fills of test_gpu_encoder_handover.py): fp16 words, bf16 words, floats"""
    rng = np.random.default_rng(seed)
    rows = M + GUARD
    return SimpleNamespace(f16=rng.integers(0x3000, 0x7000, (2, rows, N)).astype(np.uint16).view(np.float16),
                           bf=rng.integers(0x3000, 0x7000, (rows, N)).astype(np.uint16),
                           f32=rng.uniform(100, 200, (rows, N)).astype(np.float32))


def plane_cases(tile, M, n_cu):
    """every K and epilogue at one row of PLANE_TABLE; ln_scale goes round 1, 64, 1024"""
    out = []
    for K in PLANE_KS:
        for epi, period in EPILOGUES:
            out.append(make_case(0, 384, M, K, epi, n_cu, period, LN_SCALES[len(out) % 3]))
            assert out[-1].bm == (192 if tile == 1 else 256), out[-1].name
    return out


def conv2_case(family):
    """epilogue 11 in conv2's form: d_in = 32 (K = 96; the bf16 family needs K % 64 == 0: d_in = 64, K = 192), T = 100, three
    clips: the clip boundaries at rows 100 and 200 fall inside the 32-row slabs 96..127 and 192..223"""
    return make_case(family, 384, 300, 192 if family else 96, EPI_CONV, 1 if family == 0 else 0, 100, form="conv2")


def bf16_cases(N):
    out = []
    for M in BF16_ROWS[N]:
        for K in BF16_KS:
            out.append(make_case(1, N, M, K, EPI_RESIDUAL))
            out.append(make_case(1, N, M, K, EPI_CONV, pos_period=32 if K == 64 else 100))
    return out


EDGE_KINDS = ("constant", "mean_1e4", "spread_1e-3", "span_1e9")
EDGE_CONSTANT = 2.5


def edge_case(family, M=289, n_cu=1):
    """One case per family with the rows a LayerNorm gets wrong, in both tiles and both wavefront rows of each (M = 289,
    192-row tiles: rows 0..95, 96..191, 192..287 and the lone row 288).  Epilogue 5; the bias holds multiples of 1/8 so
    that `constant` rows are exact: a zero A row, R = 2.5 - bias, every finished value exactly 2.5.
      constant     variance 0, rstd = 316: the output must be ln_b bit for bit
      mean_1e4     mean 1e4, spread 1
      spread_1e-3  spread 1e-3 around 0 (zero A row)
      span_1e9     magnitudes 1e-6 ... 1e+3 (zero A row)
    Gain 0 in three columns, shift 0 in three."""
    c = make_case(family, 384, M, 64 if family else 96, EPI_RESIDUAL, n_cu if family == 0 else 0, seed=7)
    rng = np.random.default_rng(5 + family)
    c.name = "edge-" + c.name
    c.bias = (rng.integers(-16, 17, c.N) / 8.0).astype(np.float32)
    c.g[[5, 100, 383]] = 0.0
    c.b[[7, 100, 380]] = 0.0
    A = c.A.reshape(M, c.K)
    rows = {}
    for base in (3, 99, 195):
        for i, kind in enumerate(EDGE_KINDS):
            rows[base + 9 * i] = kind
    rows[M - 1] = "mean_1e4"
    rows[M - 2] = "constant"
    for r, kind in rows.items():
        if kind == "constant":
            A[r] = 0.0
            c.R[r] = np.float32(EDGE_CONSTANT) - c.bias
        elif kind == "mean_1e4":
            c.R[r] = (1e4 + rng.standard_normal(c.N)).astype(np.float32)
        elif kind == "spread_1e-3":
            A[r] = 0.0
            c.R[r] = (1e-3 * rng.standard_normal(c.N)).astype(np.float32) - c.bias
        else:
            A[r] = 0.0
            c.R[r] = (10.0 ** rng.uniform(-6, 3, c.N) * rng.choice([-1.0, 1.0], c.N)).astype(np.float32) - c.bias
    c.edge = rows
    return c


# -------------------------------------------------------------------------------------------- the float64 reference ---
def reference(c):
    """(C, LayerNorm(C) * g + b) in float64: gather rows, contract, epilogue"""
    A, W = (bf16_round(c.A), bf16_round(c.W)) if c.family else (c.A, c.W)
    x = gather_rows(A.astype(np.float64), c.M, c.K, c.a_rpb, c.a_bs, c.lda) @ W.astype(np.float64).T + c.bias.astype(np.float64)
    if c.epi & GELU:
        x = gelu(x)
    if c.epi & POS:
        x = x + c.pos.astype(np.float64)[np.arange(c.M) % c.pos.shape[0]]
    if c.epi & RESIDUAL:
        x = x + c.R.astype(np.float64)
    return x, ln64(x, c.g, c.b)


# ------------------------------------------------------------------------------------------- the float32 emulation ---
def row_sums(v, wn):
    """sum over the columns of every row of v [rows][N], float32, in the kernels' order: wavefront column wn owns N / wn
    columns as NI blocks of 32; lane l of 8 adds its columns 4 l .. 4 l + 3 of every block, the 8 lanes combine in a
    butterfly (xor 1, 2, 4), the wn partial sums are added pairwise; times float32(1 / N)"""
    rows, N = v.shape
    ni = N // (wn * 32)
    t = f32(v).reshape(rows, wn, ni, 8, 4).transpose(0, 1, 3, 2, 4).reshape(rows, wn, 8, ni * 4)
    s = np.zeros((rows, wn, 8), np.float32)
    for i in range(ni * 4):
        s = s + t[..., i]
    for sh in (1, 2, 4):
        s = s + s[..., np.arange(8) ^ sh]
    q = s[..., 0]
    tot = (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3]) if wn == 4 else q[:, 0] + q[:, 1]
    return tot * (np.float32(1.0) / np.float32(N))


def mfma_contract(a, w):
    """a [rows][K] . w [N][K]^T as the matrix cores accumulate it: one partial dot product per 32-deep MFMA step (formed
    inside the instruction; here in float64, rounded once), added to a float32 accumulator step by step.  (A BLAS sgemm
    is a chain of K float32 additions per output, 32 times as many roundings as the kernels make.)"""
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k0 in range(0, a.shape[1], 32):
        acc = acc + (a[:, k0:k0 + 32].astype(np.float64) @ w[:, k0:k0 + 32].astype(np.float64).T).astype(np.float32)
    return acc


class Emu:
    """Engine.dbg_gemm_ln_fused in float32 numpy.  defect: None, or one of DEFECTS:
      one_pass_variance    E[x^2] - mean^2 instead of the second pass
      rows_past_m          the rows of the last tile behind M are treated as rows (A clamped to row M - 1 as the kernels
                           stage it, R and the stores in the guard)
      row_map_rotated      the normalised rows leave the registers rotated by 8 inside every 32-row slab
      flag_first_wave_row  only the first wavefront row of a tile reports a non-finite row
      scale_on_lo_only     hi = fp16(y), lo = fp16(y * ln_scale - hi)"""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    def dbg_gemm_ln_fused(self, family, epi, M, N, K, A, a_rpb, a_bs, lda, W, bias, C, planes, ln_g, ln_b, ln_scale=64.0, pos=None,
                          pos_period=None, y32=None, n_cu=0):
        bm, wn, _ = geometry(family, M, N, K, epi, n_cu)
        C = np.array(C, np.float32)
        planes = np.array(planes)
        y32 = None if y32 is None else np.array(y32, np.float32)
        rows = min(-(-M // bm) * bm, C.shape[0]) if self.defect == "rows_past_m" else M
        a = gather_rows(f32(A).reshape(-1), M, K, a_rpb, a_bs, lda)[np.minimum(np.arange(rows), M - 1)]
        w = f32(W)
        if family:
            a, w = bf16_round(a), bf16_round(w)
        with np.errstate(invalid="ignore", over="ignore"):
            v = mfma_contract(a, w) + f32(bias)
            if epi & GELU:
                v = f32(0.5) * v * (f32(1.0) + erf(v / np.float32(np.sqrt(2.0))).astype(np.float32))
            if epi & POS:
                period = pos.shape[0] if pos_period is None else pos_period
                v = v + f32(pos)[np.arange(rows) % period]
            if epi & RESIDUAL:
                v = v + C[:rows]
            v = f32(v)
            C[:rows] = v
            mean = row_sums(v, wn)
            d = v - mean[:, None]
            var = row_sums(v * v, wn) - mean * mean if self.defect == "one_pass_variance" else row_sums(d * d, wn)
            bad = ~((np.abs(mean) <= np.float32(3.0e38)) & (var <= np.float32(3.0e38)))
            if self.defect == "flag_first_wave_row":
                bad &= (np.arange(rows) % bm) < bm // 2
            rstd = f32(1.0 / np.sqrt((var + np.float32(1e-5)).astype(np.float64)))  # rsqrtf: one operation, one rounding
            # (x - mean) * rstd, then one fused multiply-add with the gain and the shift (the build contracts them)
            y = f32(f32(d * rstd[:, None]).astype(np.float64) * f32(ln_g).astype(np.float64) + f32(ln_b).astype(np.float64))
            if self.defect == "row_map_rotated":
                m = np.arange(rows)
                y = y[np.minimum(m // 32 * 32 + (m % 32 + 8) % 32, rows - 1)]
            if y32 is not None:
                y32[:rows] = y
            if family:
                planes[:rows] = bf16_bits(y).reshape(rows, N)
            elif self.defect == "scale_on_lo_only":
                hi = y.astype(np.float16)
                planes[0, :rows], planes[1, :rows] = hi, (y * np.float32(ln_scale) - hi.astype(np.float32)).astype(np.float16)
            else:
                planes[0, :rows], planes[1, :rows] = exact_split(y * np.float32(ln_scale))
        return SimpleNamespace(C=C, planes=planes, y32=y32, p_out=None, flag=int(bad.any()), fused=True)


# ----------------------------------------------------------------------------------------------------------- checks ---
def launch(backend, c, want_y32=True, **over):
    """the case through the backend: C = the residual (or the fill) with NaN guard rows, the other outputs pre-filled"""
    C0 = np.full((c.M + GUARD, c.N), np.nan, np.float32)
    C0[:c.M] = c.R if c.epi & RESIDUAL else c.fills.f32[:c.M]
    a = dict(M=c.M, N=c.N, K=c.K, A=c.A, a_rpb=c.a_rpb, a_bs=c.a_bs, lda=c.lda, W=c.W, bias=c.bias, C=C0,
             planes=c.fills.bf if c.family else c.fills.f16, ln_g=c.g, ln_b=c.b, ln_scale=c.ln_scale, pos=c.pos,
             y32=c.fills.f32 if want_y32 else None, n_cu=c.n_cu)
    a.update(over)
    return C0, backend.dbg_gemm_ln_fused(c.family, c.epi, **a)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def check_planes(c, planes, y32, scale=None):
    """the planes are what the fp32 copy says, bit for bit"""
    M = c.M
    if c.family:
        assert np.array_equal(planes[:M], bf16_bits(y32[:M]).reshape(M, c.N)), c.name + ": bf16 plane != rne(ln_y32)"
    else:
        hi, lo = exact_split(y32[:M] * np.float32(c.ln_scale if scale is None else scale))
        assert np.array_equal(bits(planes[0, :M]), bits(hi)), c.name + ": hi != fp16(ln_y32 * ln_scale)"
        assert np.array_equal(bits(planes[1, :M]), bits(lo)), c.name + ": lo != fp16(ln_y32 * ln_scale - hi)"


def check(c, C0, out, margin=1.0, edge_c=EDGE_C):
    """every assertion on one fused launch; returns the worst err / bar of each check"""
    M, f = c.M, c.fills
    assert out.fused, c.name + ": the launcher did not fuse the LayerNorm"
    assert out.flag == 0, c.name + ": non-finite flag on finite rows (the NaN guard rows of R take part in nothing)"
    assert np.array_equal(bits(out.C[M:]), bits(C0[M:])), c.name + ": C written past row M"
    assert np.array_equal(bits(out.y32[M:]), bits(f.f32[M:])), c.name + ": ln_y32 written past row M"
    given = f.bf if c.family else f.f16
    assert np.array_equal(bits(out.planes[..., M:, :]), bits(given[..., M:, :])), c.name + ": LayerNorm plane written past row M"
    C64, Y64 = reference(c)
    got = out.C[:M].astype(np.float64)
    assert np.isfinite(got).all(), c.name
    res = {"C": np.abs(got - C64).max() / max(1e-30, np.abs(C64).max()) / C_BAR}
    y = out.y32[:M].astype(np.float64)
    yc = ln64(got, c.g, c.b)
    ordinary = np.ones(M, bool)
    if c.edge:
        ordinary[sorted(c.edge)] = False
    if ordinary.any():
        res["ln_of_C"] = np.abs(y - yc)[ordinary].max() / LN_OF_C_BAR
        res["chain"] = np.abs(y - Y64)[ordinary].max() / CHAIN_BAR
    if c.edge:
        e = sorted(c.edge)
        x = got[e]
        mean = x.mean(1, keepdims=True)
        rstd = 1.0 / np.sqrt(x.var(1, keepdims=True) + 1e-5)
        bound = edge_c * U * (np.abs(mean) + np.abs(x - mean).max(1, keepdims=True)) * rstd * np.abs(c.g).max() + 2 * U * np.abs(yc[e])
        res["edge"] = (np.abs(y[e] - yc[e]) / bound).max()
        for r in e:
            if c.edge[r] == "constant":
                assert np.array_equal(bits(out.C[r]), bits(np.full(c.N, EDGE_CONSTANT, np.float32))), (c.name, r, "the row is not constant")
                assert np.array_equal(bits(out.y32[r]), bits(c.b)), (c.name, r, "a constant row must give ln_b bit for bit")
    for k, v in res.items():
        assert v <= margin, (c.name, k, f"{v:.3g} of its bar, margin {margin}")
    check_planes(c, out.planes, out.y32)
    return res


def run_case(backend, c, margin=1.0, edge_c=EDGE_C, without_y32=False, scales=(), kernel=None):
    """launch + check; without_y32: a launch with ln_y32 == nullptr gives the same plane bits; scales: further ln_scale
    values, each held to the split of ITS ln_y32 * scale.  Prints the kernel reached and the measured errors."""
    C0, out = launch(backend, c)
    res = check(c, C0, out, margin, edge_c)
    print(f"{c.name}: {kernel or c.kernel}: " + ", ".join(f"{k} {v:.3g} of its bar" for k, v in res.items()))
    if without_y32:
        _, alone = launch(backend, c, want_y32=False)
        assert alone.y32 is None and alone.fused and alone.flag == 0
        assert np.array_equal(bits(alone.planes), bits(out.planes)), c.name + ": other plane bits without ln_y32"
        assert np.array_equal(bits(alone.C), bits(out.C)), c.name
    for s in scales:
        _, o = launch(backend, c, ln_scale=s)
        assert np.array_equal(bits(o.y32), bits(out.y32)), (c.name, s, "ln_y32 depends on ln_scale")
        check_planes(c, o.planes, o.y32, s)
    return res, out


def flag_checks(backend, family, N, M, n_cu):
    """The flag word.  One row of R (epilogue 5) or of pos (epilogue 11, pos_period > M: one row takes it) holds +Inf or
    -Inf: 1, for row 0, row M - 1 (alone in the second wavefront row of the ragged last tile) and a middle row.  A row of
    +-1e17 alternating (variance 1e34, finite): 0.  (Finite cases with NaN guard rows in R: 0, in check().)"""
    K = 64
    for epi in (EPI_RESIDUAL, EPI_CONV):
        c = make_case(family, N, M, K, epi, n_cu, pos_period=M + 11 if epi & POS else 0, seed=3)
        src = c.R if epi & RESIDUAL else c.pos
        C0, out = launch(backend, c)
        check(c, C0, out)
        for row in (0, M - 1, M // 2):
            keep = src[row].copy()
            for bad in (np.inf, -np.inf):
                src[row, 200 % N] = bad
                assert launch(backend, c)[1].flag == 1, (c.name, c.kernel, row, bad)
            src[row] = 1e17 * np.where(np.arange(N) % 2, -1.0, 1.0)
            got = launch(backend, c)[1]
            assert got.flag == 0 and got.fused, (c.name, c.kernel, row, "a finite variance of 1e34 raised the flag")
            src[row] = keep
    return c.kernel


def all_cases():
    """every case of the accuracy tests, in the order the tests run them"""
    out = []
    for tile, M, n_cu in PLANE_TABLE:
        out += plane_cases(tile, M, n_cu)
    out += [conv2_case(0), conv2_case(1)]
    for N in BF16_ROWS:
        out += bf16_cases(N)
    return out


def derive_edge_c():
    """the smallest power of two at which Emu stays under a quarter of the edge bound on every edge row of both families
    (and of the 256-row tile's placement of them)"""
    emu = Emu()
    for p in range(0, 16):
        try:
            for c in (edge_case(0), edge_case(0, 385, 1), edge_case(1)):
                C0, out = launch(emu, c)
                check(c, C0, out, 0.25, 2.0 ** p)
            return 2 ** p
        except AssertionError:
            continue
    raise AssertionError("no EDGE_C up to 2^15")
