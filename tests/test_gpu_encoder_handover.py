"""GPU (-m gpu): the encoder's contraction kernels under the operand and output ADDRESSING that Engine::encode_enqueue and
encode_enqueue_bf16 give them, and the two kernels that hand operands over between them (layernorm_rows_planes,
f32_to_planes), through the taps wt_dbg_gemm_addressed, wt_dbg_layernorm_planes and wt_dbg_f32_to_planes
(include/wt_debug.h).  tests/test_gpu_kernels.py holds the same kernels to float64 on contiguous operands only.

One float64 reference serves every GEMM form (expected_cells): GATHER row m of the operand from the flat buffer at
(m // a_rpb) * a_bs + (m % a_rpb) * lda, CONTRACT with W and apply the epilogue, SCATTER with the output formula of
csrc/kernels.h (rows: c_off + (m // c_rpb) * c_bs + (m % c_rpb) * ldc + n; kEpiKvLayout: its cache formula) into a copy
of the in / out buffer.  The WHOLE buffer is compared: the addressed cells to the tolerance of the contiguous test of the
same kernel and epilogue in tests/test_gpu_kernels.py, every other cell bit for bit.  Operand buffers are random
everywhere, pad rows and the slack behind the last row included, and output buffers are pre-filled with a non-zero
pattern, so a wrong row, clip offset or stride can neither read nor leave zeros.

Tolerances (none is new):  fp32 output, every family: rel_err < 3e-6 (test_gemm_epilogues, test_plane_gemm_epilogues,
test_bf16_gemm_epilogues).  Plane output: rel_err < 4e-6 on (hi + lo) / scale (test_plane_gemm_plain_and_plane_output).
bf16 output: |out - ref| <= |ref| 2^-8 + 1e-6 (test_bf16_gemm_matches_bf16_rounded_operands).  The bf16 family is held
to float64 on the bf16-rounded operands, as there.  LayerNorm's fp32 copy: 5e-6 absolute on test_layernorm's input
distribution.  Operands are drawn as in those tests: A standard normal, W standard normal / sqrt(K), bias and pos
standard normal.

Tile choice of the plane GEMM (plane_gemm_plan in k_gemm_planes.hip: cost = rows x 128-column units x rounds of n_cu CUs).
n_cu = 0, 8, 11 are the values test_plane_gemm_every_tile_shape_gives_the_same_result reaches the three tiles with at
M = 2000; at the row counts used here they pick the 192 x 128 tile except for N = 1152, M = 200 at n_cu = 8 (192 x 384).
n_cu = 1 and 2 are added because they do reach the 384-column tiles here: M = 240, N = 384: n_cu 1 -> 256 x 384 (one row
tile against two), 2 -> 192 x 384;  M = 150 or 64, N = 384: n_cu 1 -> 192 x 384;  M = 200, N = 1152: 1, 2 -> 256 x 384."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
from scipy.special import erf

from test_gpu_frontend_kernels import bf16_rne_bits, check_split

pytestmark = pytest.mark.gpu

BIAS, GELU, RESIDUAL, POS, KV = 1, 2, 4, 8, 16
CONTIGUOUS = 1 << 30   # a_rpb / c_rpb of an operand without clip structure (the launchers' default)
FP32_TOL = 3e-6
PLANE_TOL = 4e-6
N_CU = [0, 8, 11, 1, 2]
FAMILIES = [pytest.param(0, 0, id="f32-v0"), pytest.param(0, 13, id="f32-v13"), pytest.param(1, None, id="planes"),
            pytest.param(2, None, id="bf16")]


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.set_option("gemm_variant", -1)
    e.close()


def select_family(eng, kind, variant):
    eng.set_option("gemm_variant", variant if kind == 0 else -1)


def gelu(x):
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def rel_err(a, ref):
    return np.abs(a - ref).max() / max(1e-30, np.abs(ref).max())


def bf16_round(x):
    return (bf16_rne_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def bf16_bits_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


# ------------------------------------------------------------------------------------------- the float64 reference ---

def gather_rows(a_flat, M, K, a_rpb, a_bs, lda):
    m = np.arange(M)
    start = (m // a_rpb) * a_bs + (m % a_rpb) * lda
    return a_flat[start[:, None] + np.arange(K)[None, :]]


def row_major_index(M, N, c_off, c_rpb, c_bs, ldc):
    m = np.arange(M)
    return (c_off + (m // c_rpb) * c_bs + (m % c_rpb) * ldc)[:, None] + np.arange(N)[None, :]


def kv_index(M, N, c_off, T, kv_batch, kv_heads, kv_dmodel):
    """GemmArgs in csrc/kernels.h: column n = slab * d_model + head * 64 + dd, row m = b * T + t
    -> C[((slab * kv_batch + b) * kv_heads + head) * T * 64 + t * 64 + dd]"""
    m, n = np.arange(M)[:, None], np.arange(N)[None, :]
    b, t = m // T, m % T
    slab, head, dd = n // kv_dmodel, (n % kv_dmodel) // 64, n % 64
    return c_off + ((slab * kv_batch + b) * kv_heads + head) * T * 64 + t * 64 + dd


def expected_cells(c, bf16, fill32=None):
    """(flat index [M][N] of every cell the launch owns, its float64 value).  fill32: the fp32 buffer before the launch
    (the in-place residual)."""
    A, W = (bf16_round(c.A), bf16_round(c.W)) if bf16 else (c.A, c.W)
    rows = gather_rows(A.astype(np.float64), c.M, c.K_real, c.a_rpb, c.a_bs, c.lda)
    ref = rows @ W[:, :c.K_real].astype(np.float64).T + c.bias.astype(np.float64)
    if c.epi & GELU:
        ref = gelu(ref)
    if c.epi & POS:
        ref = ref + c.pos.astype(np.float64)[np.arange(c.M) % c.pos.shape[0]]
    if c.epi & KV:
        idx = kv_index(c.M, c.N, c.c_off, c.c_rpb, *c.kv)
    else:
        idx = row_major_index(c.M, c.N, c.c_off, c.c_rpb, c.c_bs, c.ldc)
    if c.epi & RESIDUAL:
        ref = ref + fill32[idx].astype(np.float64)
    return idx, ref


def make_case(name, epi, M, N, K, K_real, a_len, a_rpb, a_bs, lda, c_len, c_off, c_rpb, c_bs, ldc, pos_period=0, kv=(0, 0, 0),
              seg=0, out_scale=(64.0, 1.0, 1.0)):
    rng = np.random.default_rng(sum(name.encode()) * 1000 + M + N + K)
    W = np.zeros((N, K), np.float32)
    W[:, :K_real] = rng.standard_normal((N, K_real)) / np.sqrt(K_real)
    return SimpleNamespace(
        name=name, epi=epi, M=M, N=N, K=K, K_real=K_real, A=rng.standard_normal(a_len).astype(np.float32), a_rpb=a_rpb,
        a_bs=a_bs, lda=lda, W=W, bias=rng.standard_normal(N).astype(np.float32),
        pos=rng.standard_normal((pos_period, N)).astype(np.float32) if pos_period else None, c_len=c_len, c_off=c_off,
        c_rpb=c_rpb, c_bs=c_bs, ldc=ldc, kv=kv, seg=seg, out_scale=np.array(out_scale, np.float32),
        fill32=rng.standard_normal(c_len).astype(np.float32),
        fill16=rng.integers(0x3000, 0x7000, (2, c_len)).astype(np.uint16).view(np.float16),
        fillbf=rng.integers(0x3000, 0x7000, c_len).astype(np.uint16))


@functools.lru_cache(maxsize=None)
def conv1_case(n_mels, d, T0, clips):
    """conv1 as a GEMM over overlapping rows: row (clip, t) is rows t .. t + 2 of the clip's [T0 + 2][n_mels] block, K =
    3 n_mels padded to the k-tile under zero weights (so every row over-reads into what follows it, the last row of the
    last clip into the slack behind the buffer), output row t at padded row t + 1 of [clips][T0 + 2][d]."""
    k_real = 3 * n_mels
    K = (k_real + 63) // 64 * 64
    return make_case(f"conv1-{n_mels}-{d}-{T0}-{clips}", BIAS | GELU, clips * T0, d, K, k_real,
                     a_len=clips * (T0 + 2) * n_mels + (K - k_real), a_rpb=T0, a_bs=(T0 + 2) * n_mels, lda=n_mels,
                     c_len=clips * (T0 + 2) * d, c_off=d, c_rpb=T0, c_bs=(T0 + 2) * d, ldc=d)


@functools.lru_cache(maxsize=None)
def conv2_case(d, T0, clips):
    """conv2 with stride 2: output t reads padded rows 2 t .. 2 t + 2 of [clips][T0 + 2][d] (lda = 2 d, K = 3 d), plus
    the positional embedding of period T = T0 / 2; contiguous output with a guard row behind it."""
    T = T0 // 2
    return make_case(f"conv2-{d}-{T0}-{clips}", BIAS | GELU | POS, clips * T, d, 3 * d, 3 * d, a_len=clips * (T0 + 2) * d, a_rpb=T,
                     a_bs=(T0 + 2) * d, lda=2 * d, c_len=(clips * T + 1) * d, c_off=0, c_rpb=CONTIGUOUS, c_bs=0, ldc=d,
                     pos_period=T)


@functools.lru_cache(maxsize=None)
def qkv_case(d, M):
    return make_case(f"qkv-{d}-{M}", BIAS, M, 3 * d, d, d, a_len=M * d, a_rpb=CONTIGUOUS, a_bs=0, lda=d, c_len=(M + 1) * 3 * d,
                     c_off=0, c_rpb=CONTIGUOUS, c_bs=0, ldc=3 * d, seg=d, out_scale=(0.25, 8.0, 64.0))


@functools.lru_cache(maxsize=None)
def kv_case():
    d, heads, layers, T, clips = 128, 2, 2, 50, 3
    slab = clips * heads * T * 64
    return make_case("cross-kv", BIAS | KV, clips * T, layers * 2 * d, d, d, a_len=clips * T * d, a_rpb=CONTIGUOUS, a_bs=0, lda=d,
                     c_len=64 + (layers * 2 + 1) * slab, c_off=64, c_rpb=T, c_bs=0, ldc=0, kv=(clips, heads, d))


@functools.lru_cache(maxsize=None)
def residual_case():
    M, N, K, ldc = 200, 256, 128, 256
    return make_case("residual-padded", BIAS | RESIDUAL, M, N, K, K, a_len=M * K, a_rpb=CONTIGUOUS, a_bs=0, lda=K,
                     c_len=5 * 42 * ldc, c_off=ldc, c_rpb=40, c_bs=42 * ldc, ldc=ldc)


def launch(eng, kind, c, out, n_cu=0, **over):
    a = dict(M=c.M, N=c.N, K=c.K, A=c.A, a_rpb=c.a_rpb, a_bs=c.a_bs, lda=c.lda, W=c.W, out=out, c_off=c.c_off, c_rpb=c.c_rpb,
             c_bs=c.c_bs, ldc=c.ldc, bias=c.bias, pos=c.pos, out_scale=c.out_scale, seg=c.seg, kv=c.kv, n_cu=n_cu)
    a.update(over)
    return eng.dbg_gemm_addressed(kind, c.epi, **a)


def check_untouched(got_bits, fill_bits, idx, what):
    keep = np.ones(fill_bits.shape[-1], bool)
    keep[idx.ravel()] = False
    assert keep.sum() > 0 and idx.size == np.unique(idx).size, "the case must leave cells to guard, and own each cell once"
    assert np.array_equal(got_bits[..., keep], fill_bits[..., keep]), what + ": a cell outside the launch's own was written"


def check_fp32(eng, kind, c, n_cu=0):
    out = launch(eng, kind, c, c.fill32, n_cu)
    idx, ref = expected_cells(c, kind == 2, c.fill32)
    err = rel_err(out[idx], ref)
    print(f"{c.name} kind {kind} n_cu {n_cu}: fp32 rel_err {err:.3g} (bound {FP32_TOL})")
    check_untouched(out.view(np.uint32), c.fill32.view(np.uint32), idx, c.name)
    assert err < FP32_TOL, c.name


def check_planes(eng, c, n_cu=0):
    """kind 1, plane output: (hi + lo) / out_scale[n // seg] against float64, and hi is the fp16 value nearest to what
    the two planes reconstruct.  (Nearest, not "fp16(hi + lo) == hi" bit for bit: lo = fp16(a - hi) may round UP to exactly
    half an ulp of hi — one remainder in 8192 does — and the tie hi + lo then goes to the even neighbour, which a correct
    split's hi need not be.  The count of such ties is printed.)"""
    out = launch(eng, 1, c, c.fill16, n_cu)
    idx, ref = expected_cells(c, False)
    hi, lo = out[0][idx], out[1][idx]
    scale = c.out_scale[np.arange(c.N) // (c.seg if c.seg else c.N)].astype(np.float64)
    s = hi.astype(np.float64) + lo.astype(np.float64)
    err = rel_err(s / scale, ref)
    up, dn = np.nextafter(hi, np.float16(np.inf)).astype(np.float64), np.nextafter(hi, np.float16(-np.inf)).astype(np.float64)
    ties = int((s.astype(np.float16).view(np.uint16) != hi.view(np.uint16)).sum())
    print(f"{c.name} n_cu {n_cu}: plane rel_err {err:.3g} (bound {PLANE_TOL}), {ties} of {hi.size} hi + lo on a tie")
    check_untouched(out.view(np.uint16), c.fill16.view(np.uint16), idx, c.name)
    assert err < PLANE_TOL, c.name
    assert np.isfinite(s).all()
    assert (np.abs(lo.astype(np.float64)) <= np.abs(s - up)).all() and (np.abs(lo.astype(np.float64)) <= np.abs(s - dn)).all(), \
        c.name + ": hi is not the fp16 nearest to hi + lo"


def check_bf16(eng, c):
    out = launch(eng, 2, c, c.fillbf)
    idx, ref = expected_cells(c, True)
    got = bf16_bits_to_f32(out[idx.ravel()]).reshape(idx.shape).astype(np.float64)
    worst = (np.abs(got - ref) / (np.abs(ref) * 2.0 ** -8 + 1e-6)).max()
    print(f"{c.name}: bf16 output at most {worst:.3f} of its bound")
    check_untouched(out, c.fillbf, idx, c.name)
    assert (np.abs(got - ref) <= np.abs(ref) * 2.0 ** -8 + 1e-6).all(), c.name


def shape_id(shape):
    return "-".join(str(v) for v in shape)


def n_cu_values(kind, c):
    return N_CU if kind == 1 and c.N % 384 == 0 else [0]


# ------------------------------------------------------------------------------------------------------ GEMM forms ---

# (n_mels, d, T0, clips): a clip boundary at row 100, inside the 32-row slab 96..127 and inside a 192-row tile; c_rpb = 40,
# where slab 32..63 wraps at its row 8, N = 384; c_rpb at the contract's minimum
CONV1 = [(80, 128, 100, 3), (40, 384, 40, 6), (80, 128, 32, 5)]


@pytest.mark.parametrize("kind,variant", FAMILIES)
@pytest.mark.parametrize("shape", CONV1, ids=shape_id)
def test_conv1_form_fp32_output(eng, shape, kind, variant):
    """bias | gelu into [clips][T0 + 2][d] at c_off = d, as fp32 from every family: rows 0 and T0 + 1 of every clip come
    back as given.  The reference contracts the 3 n_mels real columns only."""
    select_family(eng, kind, variant)
    c = conv1_case(*shape)
    for n_cu in n_cu_values(kind, c):
        check_fp32(eng, kind, c, n_cu)


@pytest.mark.parametrize("shape", CONV1, ids=shape_id)
def test_conv1_form_plane_output(eng, shape):
    c = conv1_case(*shape)
    for n_cu in n_cu_values(1, c):
        check_planes(eng, c, n_cu)


@pytest.mark.parametrize("shape", CONV1, ids=shape_id)
def test_conv1_form_bf16_output(eng, shape):
    check_bf16(eng, conv1_case(*shape))


# (d, T0, clips): T = 50, K = 384; T = 32 (pos_period at its minimum), K = 1152, N = 384
@pytest.mark.parametrize("kind,variant", FAMILIES)
@pytest.mark.parametrize("shape", [(128, 100, 3), (384, 64, 2)], ids=shape_id)
def test_conv2_form(eng, shape, kind, variant):
    select_family(eng, kind, variant)
    c = conv2_case(*shape)
    for n_cu in n_cu_values(kind, c):
        check_fp32(eng, kind, c, n_cu)


@pytest.mark.parametrize("d,M", [(128, 150), (384, 200)])
def test_qkv_plane_output_with_three_scales(eng, d, M):
    """seg = d, out_scale = (0.25, 8, 64).  d = 128: N = 384, a 384-column tile spans all three segments; d = 384: a
    384-column tile is one segment."""
    c = qkv_case(d, M)
    for n_cu in n_cu_values(1, c):
        check_planes(eng, c, n_cu)


@pytest.mark.parametrize("kind,variant", FAMILIES)
def test_cross_kv_layout(eng, kind, variant):
    """bias | KvLayout: 2 heads, 2 layers (4 slabs), T = 50, 3 clips, scattered into [slab][clip][head][t][64] behind 64
    guard elements and in front of a one-slab guard; the bf16 family writes bf16.  The expected placement is the formula
    of csrc/kernels.h (kv_index), not a reshape of the product: a swapped (clip, head) or (slab, clip) order shows."""
    select_family(eng, kind, variant)
    c = kv_case()
    if kind == 2:
        check_bf16(eng, c)
    else:
        check_fp32(eng, kind, c)


@pytest.mark.parametrize("kind,variant", FAMILIES)
def test_residual_in_place_with_padded_rows(eng, kind, variant):
    """bias | residual with c_rpb = 40, c_bs = 42 ldc, M = 200, N = 256, R = C: the launcher contract's "R addressed like
    C" (the engine itself runs the residual form on contiguous rows only)."""
    select_family(eng, kind, variant)
    check_fp32(eng, kind, residual_case())


# -------------------------------------------------------------------------------------------------------- refusals ---

# name -> (kinds, output format, epilogue, what departs from a valid small launch)
REFUSALS = {
    "c_rpb=31": ((0, 1, 2), "f32", BIAS, dict(c_rpb=31)),
    "pos_period=31": ((0, 1, 2), "f32", BIAS | GELU | POS, dict(pos_period=31)),
    "lda%8": ((1, 2), "f32", BIAS, dict(lda=132)),
    "a_bs%8": ((1, 2), "f32", BIAS, dict(a_bs=64 * 128 + 4)),
    "ldc%8": ((1, 2), "f32", BIAS, dict(ldc=132)),
    "c_bs%8": ((1, 2), "f32", BIAS, dict(c_bs=66 * 128 + 4)),
    "seg%8": ((1,), "f16", BIAS, dict(seg=68)),
    "four-segments": ((1,), "f16", BIAS, dict(seg=32)),
    "kv-as-fp32": ((2,), "f32", BIAS | KV, dict(c_rpb=32, kv=(3, 2, 128))),
    "a_len-too-short": ((0, 1, 2), "f32", BIAS, dict(a_len=(95 // 32) * 64 * 128 + (95 % 32) * 128 + 128 - 1)),
}


@pytest.mark.parametrize("name,kind", [(name, kind) for name in sorted(REFUSALS) for kind in REFUSALS[name][0]])
def test_gemm_addressed_refusals(eng, pkg, name, kind):
    """WT_ERR_INVALID_ARG before anything is launched, and the output buffer is not touched.  The valid launch these
    depart from: M = 96 rows as 3 clips of 32, N = K = 128, clips 64 rows apart on both sides, buffers with room to spare."""
    _, fmt, epi, over = REFUSALS[name]
    rng = np.random.default_rng(7)
    A = rng.standard_normal(4 * 64 * 132).astype(np.float32)
    W = rng.standard_normal((128, 128)).astype(np.float32)
    c_len = 4 * 66 * 132
    out = {"f32": rng.standard_normal(c_len).astype(np.float32),
           "f16": rng.integers(0x3000, 0x7000, (2, c_len)).astype(np.uint16).view(np.float16)}[fmt]
    before = out.copy()
    a = dict(M=96, N=128, K=128, A=A, a_rpb=32, a_bs=64 * 128, lda=128, W=W, out=out, c_off=128, c_rpb=32, c_bs=66 * 128, ldc=128,
             bias=np.ones(128, np.float32), pos=np.ones((32, 128), np.float32) if epi & POS else None, copy=False)
    a.update(over)
    eng.set_option("gemm_variant", -1)
    with pytest.raises(pkg.WtError) as ei:
        eng.dbg_gemm_addressed(kind, epi, **a)
    assert ei.value.code == 1, name
    assert np.array_equal(out.view(np.uint16), before.view(np.uint16)), name
    if name == "a_len-too-short":  # one element more is the last addressed row's end: accepted
        a["a_len"] += 1
        eng.dbg_gemm_addressed(kind, epi, **a)
        assert not np.array_equal(out, before)


# ------------------------------------------------------------------------------------------------ layernorm_planes ---

LN_SCALE = 64.0
LN_GUARD = 8


def ln_input(M, d):
    rng = np.random.default_rng(M + d)
    return ((rng.standard_normal((M, d)) * 3 + 1).astype(np.float32), rng.standard_normal(d).astype(np.float32),
            rng.standard_normal(d).astype(np.float32))


def ln_fills(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0x3000, 0x7000, (2, n)).astype(np.uint16).view(np.float16), rng.integers(0x3000, 0x7000, n).astype(np.uint16),
            rng.uniform(100, 200, n).astype(np.float32))


def exact_split(a):
    """numpy's fp16 split of float32 a: hi = fp16(a), lo = fp16(a - hi), both round to nearest even (a - hi is exact)."""
    a = np.asarray(a, np.float32)
    hi = a.astype(np.float16)
    return hi, (a - hi.astype(np.float32)).astype(np.float16)


@pytest.mark.parametrize("M", [1, 7, 8, 9, 1001])
@pytest.mark.parametrize("d", [128, 384, 512])
def test_layernorm_planes(eng, d, M):
    """Eight rows per block: a lone row, a ragged last block, many blocks.  y32 against the float64 LayerNorm; hi and lo
    bit for bit the fp16 split of float32(y32 * scale); the bf16 plane bit for bit the round-to-nearest-even of y32; the
    guard behind every output as given; without y32 the same planes; the flag 0."""
    x, g, b = ln_input(M, d)
    n = M * d
    f16, fbf, f32 = ln_fills(n + LN_GUARD, d + M)
    planes, y32, flag = eng.dbg_layernorm_planes(x, g, b, LN_SCALE, f16, y32=f32)
    xd = x.astype(np.float64)
    ref = (xd - xd.mean(1, keepdims=True)) / np.sqrt(xd.var(1, keepdims=True) + 1e-5) * g + b
    err = np.abs(y32[:n].reshape(M, d) - ref).max()
    print(f"layernorm_planes M={M} d={d}: y32 |delta| {err:.3g} (bound 5e-6)")
    assert err < 5e-6
    assert flag == 0
    a = y32[:n] * np.float32(LN_SCALE)
    hi, lo = exact_split(a)
    check_split(planes[0, :n], planes[1, :n], a, f"layernorm_planes M={M} d={d}")
    assert np.array_equal(planes[0, :n].view(np.uint16), hi.view(np.uint16)), "hi != fp16(y32 * scale)"
    assert np.array_equal(planes[1, :n].view(np.uint16), lo.view(np.uint16)), "lo != fp16(y32 * scale - hi)"
    assert np.array_equal(planes[:, n:].view(np.uint16), f16[:, n:].view(np.uint16)), "plane guard written"
    assert np.array_equal(y32[n:], f32[n:]), "y32 guard written"
    alone, none, flag2 = eng.dbg_layernorm_planes(x, g, b, LN_SCALE, f16, y32=None, want_flag=False)
    assert none is None and flag2 is None and np.array_equal(alone.view(np.uint16), planes.view(np.uint16))
    # bf16 storage mode: one plane, scale unused
    pb, yb, flag = eng.dbg_layernorm_planes(x, g, b, 1.0, fbf, y32=f32, bf16=True)
    assert flag == 0 and np.array_equal(yb.view(np.uint32), y32.view(np.uint32)), "the two forms compute different rows"
    assert np.array_equal(pb[:n], bf16_rne_bits(yb[:n])), "bf16 plane != rne(y32)"
    assert np.array_equal(pb[n:], fbf[n:]) and np.array_equal(yb[n:], f32[n:]), "guard written (bf16 form)"
    pb2, _, _ = eng.dbg_layernorm_planes(x, g, b, 1.0, fbf, y32=None, bf16=True, want_flag=False)
    assert np.array_equal(pb2, pb)


@pytest.mark.parametrize("bf16", [False, True])
def test_layernorm_planes_nonfinite_flag(eng, bf16):
    """20 rows of 384 (three blocks): the flag is 1 when ONE row holds an infinity — the first, the last or a middle row
    — and stays 0 for a row of large finite values whose mean and variance are finite (+-1e17: variance 1e34)."""
    x, g, b = ln_input(20, 384)
    fill = ln_fills(20 * 384 + LN_GUARD, 5)[1 if bf16 else 0]
    assert eng.dbg_layernorm_planes(x, g, b, LN_SCALE, fill, bf16=bf16)[2] == 0
    for row in (0, 19, 9):
        for bad in (np.inf, -np.inf):
            xi = x.copy()
            xi[row, 200] = bad
            assert eng.dbg_layernorm_planes(xi, g, b, LN_SCALE, fill, bf16=bf16)[2] == 1, (row, bad)
    for row in (0, 19, 9):
        xl = x.copy()
        xl[row] = 1e17 * np.where(np.arange(384) % 2, -1.0, 1.0)
        assert eng.dbg_layernorm_planes(xl, g, b, LN_SCALE, fill, bf16=bf16)[2] == 0, row


def test_layernorm_planes_refuses_other_widths(eng, pkg):
    x, g, b = ln_input(4, 256)
    for bf16 in (False, True):
        with pytest.raises(pkg.WtError) as ei:
            eng.dbg_layernorm_planes(x, g, b, LN_SCALE, ln_fills(4 * 256 + LN_GUARD, 1)[1 if bf16 else 0], bf16=bf16)
        assert ei.value.code == 3  # the launcher's own code: WT_ERR_FORMAT


# --------------------------------------------------------------------------------------------------- f32_to_planes ---

F2P_SCALES = np.array([0.25, 8.0, 64.0], np.float32)


# the last case has 8448000 elements, more than the 8192 blocks x 256 threads x 4 elements of one grid: a second trip
# of the grid-stride loop
@pytest.mark.parametrize("M,ld,seg", [(5, 384, 128), (3, 1536, 0), (1, 4, 0), (7, 1152, 384), (5500, 1536, 0)])
def test_f32_to_planes(eng, M, ld, seg):
    """Bit for bit numpy's fp16 split of x * scales[n // seg] (powers of two: the product is exact), the guard behind both
    planes as given.  Magnitudes over four decades, so that lo is a subnormal fp16 for part of the input."""
    rng = np.random.default_rng(M + ld + seg)
    x = (rng.standard_normal((M, ld)) * 10.0 ** rng.uniform(-3, 1, (M, ld))).astype(np.float32)
    n, guard = M * ld, 8
    fill = rng.integers(0x3000, 0x7000, (2, n + guard)).astype(np.uint16).view(np.float16)
    out = eng.dbg_f32_to_planes(x, F2P_SCALES, seg, fill)
    a = x * F2P_SCALES[np.arange(ld) // (seg if seg else ld)][None, :]
    hi, lo = exact_split(a.reshape(-1))
    assert np.array_equal(out[0, :n].view(np.uint16), hi.view(np.uint16)), "hi"
    assert np.array_equal(out[1, :n].view(np.uint16), lo.view(np.uint16)), "lo"
    assert np.array_equal(out[:, n:].view(np.uint16), fill[:, n:].view(np.uint16)), "guard written"


@pytest.mark.parametrize("M,ld,seg", [(2, 6, 0), (2, 384, 130), (2, 384, 96), (0, 384, 0)],
                         ids=["ld%4", "seg%4", "four-segments", "M=0"])
def test_f32_to_planes_refusals(eng, pkg, M, ld, seg):
    with pytest.raises(pkg.WtError) as ei:
        eng.dbg_f32_to_planes(np.ones((M, ld), np.float32), F2P_SCALES, seg, np.zeros((2, M * ld + 8), np.float16))
    assert ei.value.code == 1
