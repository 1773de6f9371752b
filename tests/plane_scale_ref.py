"""Cases, float64 references, bars and a numpy emulation of the fp16-plane GEMM at LOAD-TIME scales, for
tests/test_plane_scale_reference.py (CPU) and tests/test_gpu_plane_scales.py.

The plane kernels take every operand as two fp16 planes of x * s, s a power of two that Engine::upload_weights derives
from the weights alone: s = f16_scale_for(bound), the bound 2^4 .. 2^12 above the data.  Everything here is
stated from the fp16 format and from 4.1's rules; no number comes from a kernel.

  split(x, s)        hi = fp16(x s), lo = fp16(x s - hi): what the producers and the taps do, no clamping
  delta(x, s)        per-element model of |x - (hi + lo) / s|: max(2^-22 |x|, 2^-25 / s) — a normal lo keeps 22 bits, a
                     subnormal lo rounds at 2^-25 in scaled units
  product_model      per output element: |A| delta(W)^T + delta(A) |W|^T + 2^-22 |A| |W|^T + 2^-24 |ref|
                     (the third term is the dropped lo . lo product, the last the fp32 result's own rounding)
  emulate            hi . hi + hi . lo + lo . hi on the numpy planes, exactly, / (a_scale w_scale), rounded to float32
  encoder_bounds     4.1's bound / typical / verdict rules in float64 over a read_wtw dict, in the layout of
                     wt_dbg_encoder_scales
A `gemm` argument below is anything with the signature of Engine.dbg_gemm_planes_scaled — the tap, or `emulate`."""
import functools
import math
from fractions import Fraction

import numpy as np
from scipy.special import erf

from attn_cases import KQ, f16_scale_for

F16_MAX = 65504.0
SLACK = 4096.0       # Engine::kF16Slack
MEL_BOUND = 8.0      # Engine::kMelBound
GUARD = 8            # rows behind row M in every output: the kernels mask rows >= M

# ------------------------------------------------------------------------------------------- split and models ---


def split(x, s):
    """(hi, lo) float16 of float32 x times the power of two s; an element past fp16's range gives hi = inf, lo = -inf"""
    v = np.asarray(x, np.float32) * np.float32(s)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def delta(x, s):
    return np.maximum(2.0 ** -22 * np.abs(np.asarray(x, np.float64)), 2.0 ** -25 / float(s))


def product_model(A, W, a_scale, w_scale, ref):
    a, w = np.abs(A.astype(np.float64)), np.abs(W.astype(np.float64))
    return a @ delta(W, w_scale).T + delta(A, a_scale) @ w.T + 2.0 ** -22 * (a @ w.T) + 2.0 ** -24 * np.abs(ref)


def gelu(x):
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def f16_scale_exact(bound):
    """kernels.h's contract in exact arithmetic: the largest power of two s with bound * s <= 16384, clamped to 2^+-24; 1
    for a bound that is not positive (NaN included)"""
    bound = float(np.float32(bound))
    if not bound > 0:
        return 1.0
    if math.isinf(bound):
        return 2.0 ** -24
    b = Fraction(bound)
    for e in range(24, -24, -1):
        if b * Fraction(2) ** e <= 16384:
            return 2.0 ** e
    return 2.0 ** -24


def scale_sweep_bounds():
    """2^e for e in [-140, 127] with both float32 neighbours of each, and 0, -1, NaN, +inf"""
    out = [0.0, -1.0, float("nan"), float("inf")]
    for e in range(-140, 128):
        p = np.float32(2.0 ** e)
        out += [float(np.nextafter(p, np.float32(0))), float(p), float(np.nextafter(p, np.float32(np.inf)))]
    return out


# -------------------------------------------------------------------------------------------------- emulation ---

def emulate(A, W, bias, out, a_scale, w_scale, epi=1, out_scale=None, seg=0, n_cu=0, mutant=None):
    """The plane GEMM's arithmetic on numpy planes, with the tap's signature.  mutant: None, or one defect —
    "flush": a subnormal lo is read as zero; "scale0": out_scale[0] for every segment; "saturate": the split clamps to
    +-65504 where the format gives inf."""
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    (M, K), N = A.shape, W.shape[0]

    def planes(x, s):
        hi, lo = split(x, s)
        if mutant == "saturate":
            v = np.clip(np.asarray(x, np.float32) * np.float32(s), -F16_MAX, F16_MAX)
            hi = v.astype(np.float16)
            lo = (v - hi.astype(np.float32)).astype(np.float16)
        if mutant == "flush":
            lo = np.where(np.abs(lo) < np.float16(2.0 ** -14), np.float16(0), lo)
        return hi.astype(np.float64), lo.astype(np.float64)

    ah, al = planes(A, a_scale)
    wh, wl = planes(W, w_scale)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = (ah @ wh.T + ah @ wl.T + al @ wh.T) / (float(a_scale) * float(w_scale))
        acc = acc + np.asarray(bias, np.float64)
        if epi & 2:
            acc = gelu(acc)
        out = np.array(out, order="C")
        if out.dtype == np.float32:
            if epi & 4:
                acc = acc + out[:M].astype(np.float64)
            out[:M] = acc.astype(np.float32)
            return out
        sc = np.asarray(out_scale if out_scale is not None else [1.0, 1.0, 1.0], np.float64)
        col = np.zeros(N, int) if mutant == "scale0" else np.arange(N) // (seg if seg else N)
        if mutant == "saturate":
            v = np.clip(acc.astype(np.float32) * sc[col].astype(np.float32), -F16_MAX, F16_MAX)
            hi = v.astype(np.float16)
            lo = (v - hi.astype(np.float32)).astype(np.float16)
        else:
            hi, lo = split(acc.astype(np.float32) * sc[col].astype(np.float32), 1.0)
        out[0, :M], out[1, :M] = hi, lo
    return out


# ------------------------------------------------------------------------------------------------------ cases ---

J_INSIDE, J_OUTSIDE = (0, 6, 12), (15, 18)
G1_SHAPES = [(193, 128, 96), (193, 384, 384), (257, 384, 416)]
G_SHAPE = (193, 384, 384)  # G2, G3, G4
# (M, N) -> {n_cu: tile}: what plane_gemm_plan's cost model picks at these row counts (tile 0 = 192 x 128, 1 = 192 x 384,
# 2 = 256 x 384).  At 193 rows one CU takes the single 256-row tile, two CUs one 192-row tile each and the
# whole chip the twelve narrow ones; 257 rows are two row tiles of either height, so the taller tile never wins there;
# 128 columns have only the narrow tile.  The tests assert this table against the launcher's own plan function.
TILES = {(193, 128): {0: 0}, (193, 384): {0: 0, 2: 1, 1: 2}, (257, 384): {0: 0, 2: 1}}


def scale_at(x, j):
    """the engine's rule at a bound 2^j above the data: f16_scale_for(2^j max|x|), float32 as the engine forms it"""
    return f16_scale_for(np.float32(2.0 ** j) * np.float32(np.abs(x).max()))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def operands(M, N, K, wide=False):
    """A ~ N(0, 1), W ~ N(0, 1 / K), bias ~ N(0, 1), residual N(0, 3) + 0.7 [M + GUARD][N] (guard rows a fill the launch
    must leave alone), and the float64 products.  wide (G2): A[:, k] *= 2^-(k mod 11), W[:, k] *= 2^(k mod 11) — every k
    contributes alike while A's small columns sit up to 2^-10 under its maximum."""
    rng = np.random.default_rng(1000003 * M + 1009 * N + K + (7 if wide else 0))
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    if wide:
        A *= (2.0 ** -(np.arange(K) % 11)).astype(np.float32)
        W *= (2.0 ** (np.arange(K) % 11)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    R = (rng.standard_normal((M + GUARD, N)) * 3 + 0.7).astype(np.float32)
    prod = A.astype(np.float64) @ W.astype(np.float64).T + bias
    return _frozen(A, W, bias, R, prod)


def fill32(M, N):
    return np.random.default_rng(M + N).uniform(100, 200, (M + GUARD, N)).astype(np.float32)


def fill16(M, N):
    return np.random.default_rng(M * N).integers(0x3000, 0x7000, (2, M + GUARD, N)).astype(np.uint16).view(np.float16)


def check_guard(out, given, M, what):
    u = np.uint32 if out.dtype == np.float32 else np.uint16
    assert np.array_equal(out[..., M:, :].view(u), given[..., M:, :].view(u)), f"{what}: guard rows written"


def worst(err, bar):
    r = err / bar
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), tuple(int(v) for v in i)


def run_f32(gemm, shape, j, epi, n_cu=0, wide=False, frac=1.0):
    """One fp32-output launch of G1 / G2 against its bar times `frac`; returns error / bar at the worst element.
    Bars: j <= 12 on N(0, 1) operands the sibling tests' own, 2e-6 max|ref| (3e-6 with the residual), nothing added for
    the slack; j > 12 and the wide operands 2 x product_model element by element."""
    M, N, K = shape
    A, W, bias, R, prod = operands(M, N, K, wide)
    sa, sw = scale_at(A, j), scale_at(W, 0)
    given = R if epi & 4 else fill32(M, N)
    ref = prod + R[:M] if epi & 4 else prod
    out = gemm(A, W, bias, given, sa, sw, epi=epi, n_cu=n_cu)
    what = f"{'G2' if wide else 'G1'} {shape} j={j} epi={epi} n_cu={n_cu}"
    check_guard(out, given, M, what)
    assert np.isfinite(out[:M]).all(), what
    err = np.abs(out[:M].astype(np.float64) - ref)
    if wide or j > 12:
        bar = 2.0 * product_model(A, W, sa, sw, ref)
    else:
        bar = np.full_like(ref, (3e-6 if epi & 4 else 2e-6) * np.abs(ref).max())
    ratio, at = worst(err, bar)
    assert ratio <= frac, f"{what}: error {err[at]:.3e} at {at} is {ratio:.3f} of the bar {bar[at]:.3e} (allowed {frac})"
    return ratio


G3_FORMS = {"qkv-12-0-6": (128, (12, 0, 6)), "one-j0": (0, (0,)), "one-j6": (0, (6,)), "one-j12": (0, (12,))}
G3_A_J = 6  # the A operand of G3 sits at a mid-slack engine scale; G1 and G2 walk that ladder


def g3_scales(ref, seg, js):
    N = ref.shape[1]
    sc = [1.0, 1.0, 1.0]
    for i, j in enumerate(js):
        sc[i] = scale_at(ref[:, i * seg:(i + 1) * seg] if seg else ref, j)
    return np.array(sc, np.float32), np.arange(N) // (seg if seg else N)


def run_planes(gemm, form, epi, n_cu=0, frac=1.0):
    """One plane-output launch of G3: (hi + lo) / out_scale against 4e-6 max|ref| (the sibling plane-output bar) +
    delta(ref, out_scale), times frac; hi the fp16 nearest to hi + lo; guard rows as given.  Returns (ratio, ties)."""
    M, N, K = G_SHAPE
    A, W, bias, _, prod = operands(M, N, K)
    ref = gelu(prod) if epi & 2 else prod
    seg, js = G3_FORMS[form]
    sc, col = g3_scales(ref, seg, js)
    given = fill16(M, N)
    out = gemm(A, W, bias, given, scale_at(A, G3_A_J), scale_at(W, 0), epi=epi, out_scale=sc, seg=seg, n_cu=n_cu)
    what = f"G3 {form} epi={epi} n_cu={n_cu}"
    check_guard(out, given, M, what)
    hi, lo = out[0, :M], out[1, :M]
    s = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.isfinite(s).all(), what
    err = np.abs(s / sc[col].astype(np.float64) - ref)
    bar = 4e-6 * np.abs(ref).max() + np.maximum(2.0 ** -22 * np.abs(ref), 2.0 ** -25 / sc[col].astype(np.float64))  # + delta(ref, out_scale)
    ratio, at = worst(err, bar)
    assert ratio <= frac, f"{what}: error {err[at]:.3e} at {at} is {ratio:.3f} of the bar {bar[at]:.3e} (allowed {frac})"
    up, dn = np.nextafter(hi, np.float16(np.inf)).astype(np.float64), np.nextafter(hi, np.float16(-np.inf)).astype(np.float64)
    ties = int((s.astype(np.float16).view(np.uint16) != hi.view(np.uint16)).sum())
    al = np.abs(lo.astype(np.float64))
    assert (al <= np.abs(s - up)).all() and (al <= np.abs(s - dn)).all(), what + ": hi is not the fp16 nearest to hi + lo"
    return ratio, ties


def run_g4_operand(gemm, n_cu=0, **kw):
    """One element of A at 8 x the bound its scale was made for: hi = +inf, lo = -inf in the planes.  Every other row is
    bit for bit the launch without it; its own row is non-finite wherever the weight at that k is not zero."""
    M, N, K = G_SHAPE
    A, W, bias, _, _ = operands(M, N, K)
    sa, sw = scale_at(A, 0), scale_at(W, 0)
    r, k = 101, 37
    B = A.copy()
    B[r, k] = np.float32(8.0) * np.float32(np.abs(A).max())
    hi, lo = split(B[r, k], sa)
    assert hi.view(np.uint16) == 0x7c00 and lo.view(np.uint16) == 0xfc00
    given = fill32(M, N)
    base = gemm(A, W, bias, given, sa, sw, epi=1, n_cu=n_cu, **kw)
    out = gemm(B, W, bias, given, sa, sw, epi=1, n_cu=n_cu, **kw)
    others = np.arange(M + GUARD) != r
    assert np.array_equal(out[others].view(np.uint32), base[others].view(np.uint32)), "G4: a row without the element changed"
    assert np.isfinite(base[:M]).all()
    live = W[:, k] != 0
    assert live.sum() >= N - 1
    assert not np.isfinite(out[r, live]).any(), "G4: an out-of-range operand gave a finite result (saturated, not inf)"


def run_g4_output(gemm, n_cu=0, **kw):
    """Plane output with a column past 65504 / out_scale (through its bias): every hi word of it is inf, 0x7c00 — not the
    saturated 0x7bff — and every other column is bit for bit the launch with the small bias."""
    M, N, K = G_SHAPE
    A, W, bias, _, prod = operands(M, N, K)
    sc, _ = g3_scales(prod, 0, (0,))
    n = 200
    big = bias.copy()
    big[n] = np.float32(4.0 * F16_MAX / float(sc[0]))
    assert ((prod[:, n] - bias[n] + big[n]) * float(sc[0]) > 2 * F16_MAX).all()
    given = fill16(M, N)
    sa, sw = scale_at(A, G3_A_J), scale_at(W, 0)
    base = gemm(A, W, bias, given, sa, sw, epi=1, out_scale=sc, n_cu=n_cu, **kw).view(np.uint16)
    out = gemm(A, W, big, given, sa, sw, epi=1, out_scale=sc, n_cu=n_cu, **kw).view(np.uint16)
    words = np.unique(out[0, :M, n])
    assert list(words) == [0x7c00], f"G4: hi words {[hex(w) for w in words]} where the format gives inf (0x7c00)"
    others = np.arange(N) != n
    assert np.array_equal(out[:, :, others], base[:, :, others]), "G4: a column without the large bias changed"
    assert np.array_equal(out[:, M:], given.view(np.uint16)[:, M:])


def g4_convert_case():
    """x [M][ld], scales, seg for f32_to_planes, the cell pushed past 65504 / its segment's scale, and the pushed copy"""
    M, ld, seg = 37, 384, 128
    x = np.random.default_rng(4).standard_normal((M, ld)).astype(np.float32)
    sc = np.array([scale_at(x[:, i * seg:(i + 1) * seg], j) for i, j in enumerate((12, 0, 6))], np.float32)
    cell = (20, 130)  # segment 1, the tightest scale
    y = x.copy()
    y[cell] = np.float32(-8.0) * np.float32(np.abs(x[:, seg:2 * seg]).max())
    return x, y, sc, seg, cell


def convert_emulation(x, scales, seg, planes, mutant=None):
    """launch_f32_to_planes on numpy: with Engine.dbg_f32_to_planes' signature"""
    x = np.asarray(x, np.float32)
    M, ld = x.shape
    v = x * np.asarray(scales, np.float32)[np.arange(ld) // (seg if seg else ld)]
    if mutant == "saturate":
        v = np.clip(v, -F16_MAX, F16_MAX)
    hi, lo = split(v, 1.0)
    out = np.array(planes, np.float16, order="C")
    out[0, :M * ld], out[1, :M * ld] = hi.ravel(), lo.ravel()
    return out


def run_g4_convert(convert, **kw):
    x, y, sc, seg, cell = g4_convert_case()
    n = x.size
    given = np.random.default_rng(5).integers(0x3000, 0x7000, (2, n + 8)).astype(np.uint16).view(np.float16)
    base = convert(x, sc, seg, given, **kw).view(np.uint16)
    out = convert(y, sc, seg, given, **kw).view(np.uint16)
    at = cell[0] * x.shape[1] + cell[1]
    assert out[0, at] == 0xfc00, f"G4: hi word {hex(out[0, at])} where the format gives -inf (0xfc00)"
    others = np.arange(n + 8) != at
    assert np.array_equal(out[:, others], base[:, others])
    hi, lo = split(x * sc[np.arange(x.shape[1]) // seg], 1.0)
    assert np.array_equal(base[0, :n], hi.ravel().view(np.uint16)) and np.array_equal(base[1, :n], lo.ravel().view(np.uint16))


# ------------------------------------------------------------------------------------------- the bounds model ---

class Op:
    """one contraction operand: per-channel bound, typical magnitude"""

    def __init__(self, bound, typ):
        self.bound, self.typ = np.atleast_1d(np.asarray(bound, np.float64)), float(typ)

    @property
    def max(self):
        return float(self.bound.max())

    @property
    def ok(self):
        return not self.max > SLACK * self.typ

    @property
    def slack_bits(self):
        return math.log2(SLACK * self.typ / self.max)


def encoder_bounds(dims, t):
    """4.1's rules in float64.  Returns SimpleNamespace(records [n][10] in wt_dbg_encoder_scales' layout, ops: name -> Op
    for every tap name of fp64_encoder.encoder_fp64 plus "mel", scales: name -> the scale that operand's planes take,
    min_slack_bits, fallbacks)."""
    import types
    f = lambda k: np.asarray(t[k], np.float64)
    d, L = int(dims["n_audio_state"]), int(dims["n_audio_layer"])

    def ln_op(p):
        g, b = f(p + ".weight"), f(p + ".bias")
        return Op(np.abs(g) * math.sqrt(d - 1) + np.abs(b), math.sqrt((g * g).mean() + (b * b).mean()))

    def linear_op(w, bias, inp):
        # a Linear [N][K] pairs column k with input channel k; a conv tensor [co][ci][3] pairs column 3 ci + tap with
        # channel ci (conv1's input, the mel, has one bound for all channels)
        taps = w.shape[2] if w.ndim == 3 else 1
        w = w.reshape(w.shape[0], -1)
        inb = np.repeat(inp.bound if inp.bound.size > 1 else np.full(w.shape[1] // taps, inp.bound[0]), taps)
        bound = np.abs(w) @ inb + (np.abs(bias) if bias is not None else 0.0)
        return Op(bound, math.sqrt((w * w).sum() / w.shape[0]) * inp.typ)

    def gelu_op(o):
        return Op(np.maximum(o.bound, 0.17), 0.5 * o.typ)

    ops, scales, rec, slack = {}, {}, [], []

    def gemm(name, inp, wmax):
        a, w = f16_scale_for(np.float32(inp.max)), f16_scale_for(np.float32(wmax))
        ops[name], scales[name] = inp, a
        slack.append(inp.slack_bits)
        rec.append([a, w, float(inp.ok), inp.max, inp.typ, 0, 0, 0, 0, 0])

    wmax = lambda *names: max(float(np.abs(t[n]).max()) for n in names)
    mel = Op(MEL_BOUND, 1.0)
    gemm("mel", mel, wmax("encoder.conv1.weight"))
    c1 = f("encoder.conv1.weight")
    h1 = gelu_op(linear_op(c1, f("encoder.conv1.bias"), mel))
    gemm("h1", h1, wmax("encoder.conv2.weight"))
    kq = float(KQ)
    for l in range(L):
        p = f"encoder.blocks.{l}"
        ln1 = ln_op(p + ".attn_ln")
        gemm(f"ln1.{l}", ln1, wmax(p + ".attn.query.weight", p + ".attn.key.weight", p + ".attn.value.weight"))
        q = linear_op(f(p + ".attn.query.weight"), f(p + ".attn.query.bias"), ln1)
        k = linear_op(f(p + ".attn.key.weight"), None, ln1)
        v = linear_op(f(p + ".attn.value.weight"), f(p + ".attn.value.bias"), ln1)
        qs = Op(q.bound * kq, q.typ * kq)  # q as the kernel splits it
        for name, o in ((f"q.{l}", qs), (f"k.{l}", k), (f"v.{l}", v)):
            ops[name], scales[name] = o, f16_scale_for(np.float32(o.max))
            slack.append(o.slack_bits)
        rec.append([scales[f"q.{l}"], scales[f"k.{l}"], scales[f"v.{l}"], float(qs.ok and k.ok and v.ok),
                    qs.max, qs.typ, k.max, k.typ, v.max, v.typ])
        gemm(f"attn.{l}", v, wmax(p + ".attn.out.weight"))  # a convex combination of V rows
        ln2 = ln_op(p + ".mlp_ln")
        gemm(f"ln2.{l}", ln2, wmax(p + ".mlp.0.weight"))
        hb = gelu_op(linear_op(f(p + ".mlp.0.weight"), f(p + ".mlp.0.bias"), ln2))
        gemm(f"hidden.{l}", hb, wmax(p + ".mlp.2.weight"))
    lnp = ln_op("encoder.ln_post")
    n_text = int(dims["n_text_layer"])
    gemm("ln_post", lnp, wmax(*[f"decoder.blocks.{l}.cross_attn.{m}.weight" for l in range(n_text) for m in ("key", "value")]))
    records = np.array(rec, np.float64)
    ok = np.array([r[3] if i >= 2 and (i - 2) % 5 == 1 and i < 2 + 5 * L else r[2] for i, r in enumerate(rec)], bool)
    return types.SimpleNamespace(records=records, ok=ok, ops=ops, scales=scales, min_slack_bits=min(slack),
                                 fallbacks=int((~ok).sum()))


def is_attention(i, n):
    """record i of n is an attention record"""
    return 2 <= i < n - 1 and (i - 2) % 5 == 1


def near_boundary(x, rel=2.0 ** -18):
    """x within `rel` relative of a power of two"""
    m, _ = math.frexp(x)  # [0.5, 1)
    return min(m - 0.5, 1.0 - m) / m < rel


# The four variants of the issue, and one more: on micro (d = 128) a row outlier of a projection can raise bound / typical
# by at most sqrt(128) = 3.5 bits (the typical magnitude is an rms over the rows, which the outlier row joins), so
# v_row_scale = 1e4 — which flags layer 0's attention and out-projection on tiny, d = 384 with less slack to begin with —
# leaves 1.84 bits here and flags nothing.  A BIAS outlier enters the bound and not the typical magnitude: the fifth variant
# sets one value-projection bias of layer 0 to 1e4 (and shrinks its out-projection column alike) and does flag those two.
WEIGHT_VARIANTS = ["as-generated", "outliers", "v-row-1e4", "trained-like", "v-bias-1e4"]
# contractions the float64 model sends off the plane kernels on the micro dims (d = 128, 2 layers): indices into the
# records, conv1 0, conv2 1, layer l: qkv 2 + 5 l, attention 3 + 5 l, out 4 + 5 l, fc1 5 + 5 l, fc2 6 + 5 l, cross-KV 12
EXPECTED_FALLBACKS = {"as-generated": [], "outliers": [], "v-row-1e4": [], "trained-like": [], "v-bias-1e4": [3, 4]}


def write_variant(name, src_wtw, dst_wtw):
    from wtw import adversarial_weights, read_wtw, trained_like_weights, write_wtw
    if name == "as-generated":
        dims, t = read_wtw(src_wtw)
        write_wtw(dst_wtw, dims, {k: np.array(v) for k, v in t.items()})
    elif name == "outliers":
        adversarial_weights(src_wtw, dst_wtw, ln_gain=30.0, heavy=True)
    elif name == "v-row-1e4":
        adversarial_weights(src_wtw, dst_wtw, ln_gain=1.0, heavy=False, v_row_scale=1.0e4)
    elif name == "trained-like":
        trained_like_weights(src_wtw, dst_wtw)
    elif name == "v-bias-1e4":
        dims, t = read_wtw(src_wtw)
        t = {k: np.array(v) for k, v in t.items()}
        t["encoder.blocks.0.attn.value.bias"][77] = 1.0e4
        t["encoder.blocks.0.attn.out.weight"][:, 77] /= 1.0e4
        write_wtw(dst_wtw, dims, t)
    else:
        raise KeyError(name)


def sound_mels(dims, t, seed=0):
    """the mel inputs of the sound-bounds check, all inside [-8, 8]: uniform(-1, 1.5), uniform(-8, 8), and for three
    conv1 channels c the mel 8 sign(conv1 weight of channel c, tap 1) at every frame — the input that drives that
    channel's centre tap to its bound"""
    nm, T0 = int(dims["n_mels"]), 2 * int(dims["n_audio_ctx"])
    rng = np.random.default_rng(seed)
    mels = {"uniform(-1, 1.5)": rng.uniform(-1.0, 1.5, (nm, T0)), "uniform(-8, 8)": rng.uniform(-8.0, 8.0, (nm, T0))}
    w = np.asarray(t["encoder.conv1.weight"], np.float64)
    for c in (0, 5, int(dims["n_audio_state"]) - 1):
        s = np.where(w[c, :, 1] >= 0, 1.0, -1.0)
        mels[f"8 sign(conv1[{c}])"] = np.repeat(MEL_BOUND * s[:, None], T0, axis=1)
    return mels
