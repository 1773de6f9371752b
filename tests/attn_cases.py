"""Inputs, float64 reference and tolerances of tests/test_gpu_encoder_attention.py.  They live here, away from the GPU
tests, so that tests/test_encoder_attention_reference.py can hold them to a plain float32 attention without a GPU: a
bar that an honest fp32 implementation of the same operation misses would say nothing about the kernels.

The operation: out = softmax(q k^T / 8) v per (clip, head), d_head 64.  qkv is [B * T (+ guard rows)][3 * 64 * H],
q | k | v thirds with the heads' 64 columns inside each third; out is [B * T][64 * H]."""
import functools
import math

import numpy as np

KQ = np.float32(0.125 * 1.44269504088896340736)  # d_head^-1/2 * log2(e): what the qkv GEMM folds into the q planes

# name -> (kind, variant) of wt_dbg_encoder_attention_at
FORMS = {"f32-v0": (0, 0), "split-v1": (0, 1), "planes": (1, 0), "bf16": (2, 0)}

# (B, T, H, grid blocks): lengths below, at and one past the 64-key tile and the 128-query block, T = 1, and grids of
# every residue mod 8 (the kernels permute blockIdx by XCD with a formula that depends on gridDim.x & 7)
SWEEP = [(1, 1, 1, 1), (3, 1, 1, 3), (1, 2, 2, 2), (5, 15, 1, 5), (1, 16, 6, 6), (7, 17, 1, 7), (1, 31, 8, 8), (3, 33, 3, 9),
         (2, 63, 5, 10), (11, 65, 1, 11), (2, 127, 6, 12), (13, 128, 1, 13), (1, 129, 7, 14), (1, 257, 5, 15),
         (5, 191, 3, 30), (3, 193, 5, 30), (37, 130, 6, 444)]

SCALE_SHAPES = [(2, 100, 2), (1, 193, 3)]
# name -> (slack exponents j of the q, k, v bounds, log2 of the factor on V)
SCALE_CASES = {"j0": ((0, 0, 0), 0), "j6": ((6, 6, 6), 0), "j12": ((12, 12, 12), 0), "j12-0-6": ((12, 0, 6), 0),
               "v-times-2^8": ((0, 0, 0), 8), "v-times-2^-10": ((0, 0, 0), -10)}

ISOLATION_SHAPES = [(3, 65, 3), (2, 130, 2)]


def f16_scale_for(bound):
    """csrc/kernels.h: the largest power of two s with bound * s <= 16384, clamped to 2^+-24; 1 for a bound that is not
    positive.  (From the float32 bound's own exponent, as the engine's: no quotient that could overflow.)"""
    bound = float(np.float32(bound))
    if not bound > 0:
        return 1.0
    if math.isinf(bound):
        return 2.0 ** -24
    m, e = math.frexp(bound)  # bound = m 2^e, m in [0.5, 1): m 2^14 <= 2^14, and one more doubling fits only for m = 0.5
    return 2.0 ** max(-24, min(24, 14 - e + (1 if m == 0.5 else 0)))


def bf16_round(x):
    """round-to-nearest-even to bf16, as float32 (what the bf16 storage mode keeps in memory)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def thirds(qkv, B, T, H, dtype):
    x = np.asarray(qkv)[:B * T].astype(dtype).reshape(B, T, 3, H, 64)
    return x[:, :, 0], x[:, :, 1], x[:, :, 2]


def attention(qkv, B, T, H, dtype=np.float64):
    """softmax(q k^T / 8) v per (clip, head) over the first B * T rows, in `dtype` throughout -> [B * T][64 * H]"""
    q, k, v = thirds(qkv, B, T, H, dtype)
    s = np.einsum("bthd,bshd->bhts", q, k) / dtype(8.0)
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    out = np.einsum("bhts,bshd->bthd", p, v)
    assert out.dtype == dtype
    return out.reshape(B * T, 64 * H)


def reference_input(form, qkv):
    """what the form's reference is taken on: the bf16 storage mode is held to float64 on the bf16-rounded input"""
    return bf16_round(qkv) if form == "bf16" else np.asarray(qkv, np.float32)


def tolerances(form, ref, qkv_ref, B, T, H):
    """[B][H]: the bar of test_encoder_attention / test_encoder_attention_planes (2e-5) and of
    test_encoder_attention_bf16_storage (2^-8 max|ref| + 4e-3), made aware of V's magnitude: both were set on
    standard-normal V, and every error term of the kernels is proportional to V."""
    v = np.abs(thirds(qkv_ref, B, T, H, np.float64)[2]).max(axis=(1, 3))
    vm = np.maximum(1.0, v)
    if form == "bf16":
        return 2.0 ** -8 * np.abs(ref.reshape(B, T, H, 64)).max(axis=(1, 3)) + 4e-3 * vm
    return 2e-5 * vm


def check(form, got, qkv, B, T, H, what):
    """got [B * T][64 * H] against the float64 reference of the form, per (clip, head).  Returns (largest error, largest
    error / tolerance)."""
    x = reference_input(form, qkv)
    ref = attention(x, B, T, H)
    return check_against(form, got, ref, x, B, T, H, what)


def check_against(form, got, ref, qkv_ref, B, T, H, what):
    got = np.asarray(got)[:B * T]
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got.astype(np.float64) - ref).reshape(B, T, H, 64).max(axis=(1, 3))
    tol = tolerances(form, ref, qkv_ref, B, T, H)
    worst = tuple(int(i) for i in np.unravel_index(np.argmax(err / tol), err.shape))
    print(f"[attn-err] {what} form={form} max_err={err.max():.3e} worst_ratio={(err / tol).max():.3f} at (b, h)={worst}")
    assert (err < tol).all(), f"{what}: (clip, head) {worst}: error {err[worst]:.3e} against {tol[worst]:.3e}"
    return err.max(), (err / tol).max()


@functools.lru_cache(maxsize=None)
def normal_case(B, T, H):
    """standard-normal qkv [B * T][3 * 64 * H] with its two float64 references: (qkv, {False: (input, ref), True: the same
    on the bf16-rounded input})"""
    qkv = np.random.default_rng(B * 100000 + T * 100 + H).standard_normal((B * T, 3 * 64 * H)).astype(np.float32)
    refs = {}
    for bf in (False, True):
        x = bf16_round(qkv) if bf else qkv
        refs[bf] = (x, attention(x, B, T, H))
        refs[bf][1].setflags(write=False)
    qkv.setflags(write=False)
    return qkv, refs


def data_maxima(qkv, B, T, H):
    """(max |q| * KQ, max |k|, max |v|) over the first B * T rows, in float32 as the taps form them"""
    d = 64 * H
    a = np.abs(np.asarray(qkv, np.float32)[:B * T])
    return (np.float32(a[:, :d].max()) * KQ, np.float32(a[:, d:2 * d].max()), np.float32(a[:, 2 * d:].max()))


def plane_scales(qkv, B, T, H, j=(0, 0, 0)):
    """{q, k, v, out} as Engine::load_weights forms them: f16_scale_for of a bound 2^j above the data maximum; the out
    scale is the v scale (sl.out comes from vo.bound)"""
    m = data_maxima(qkv, B, T, H)
    s = [f16_scale_for(np.float32(2.0 ** j[i]) * m[i]) for i in range(3)]
    return np.array(s + [s[2]], np.float32)


@functools.lru_cache(maxsize=None)
def scale_case(B, T, H, log2_v):
    qkv = normal_case(B, T, H)[0].copy()
    qkv[:, 2 * 64 * H:] *= np.float32(2.0 ** log2_v)
    ref = attention(qkv, B, T, H)
    qkv.setflags(write=False)
    ref.setflags(write=False)
    return qkv, ref


# ------------------------------------------------------------------------------------------------- softmax edges ---

def _dominant(T, j_star):
    rng = np.random.default_rng(1000 * T + j_star)
    qkv = rng.standard_normal((T, 192)).astype(np.float32)
    u = rng.standard_normal(64)
    qkv[:, 0:64] = u + 0.05 * rng.standard_normal((T, 64))
    return qkv, u


def edge_case(name):
    """(T, qkv [T][192], expected): one clip, one head.  expected is None, or "v0" / "mean": the closed form every
    output row must equal besides the float64 reference (edge_expected)."""
    part = name.split("-")
    if part[0] == "dominant":  # every query sees key j* about 6 |u|^2 / 8 = 48 above the rest
        T, j_star = int(part[1][1:]), int(part[2][1:])
        qkv, u = _dominant(T, j_star)
        qkv[j_star, 64:128] = 6.0 * u
        return T, qkv, None
    if name == "key0-alone":  # 40 |u|^2 / 8 = 320 above the rest: every other probability underflows, in every tile
        T = 130
        qkv, u = _dominant(T, 0)
        qkv[0, 64:128] = 40.0 * u
        return T, qkv, "v0"
    if part[0] == "qzero":  # equal scores: the mean of V
        T = int(part[1][1:])
        qkv = np.random.default_rng(T).standard_normal((T, 192)).astype(np.float32)
        qkv[:, 0:64] = 0.0
        return T, qkv, "mean"
    if name == "falling-ramp":  # the mirror of test_encoder_attention_planes_deferred_maximum: 9 log2 units DOWN per tile
        T = 400
        qkv = (np.random.default_rng(9).standard_normal((T, 192)) * 0.05).astype(np.float32)
        qkv[:, 0:64] += 1.0
        ramp = -9.0 / (64 * 1.4426950408889634) * np.arange(T)
        qkv[:, 64:128] += (ramp / 8.0)[:, None].astype(np.float32)
        return T, qkv, None
    raise KeyError(name)


EDGE_CASES = ["dominant-T65-k0", "dominant-T65-k63", "dominant-T65-k64", "dominant-T100-k99", "dominant-T129-k64",
              "dominant-T129-k128", "key0-alone", "qzero-T1", "qzero-T65", "qzero-T130", "falling-ramp"]


def edge_expected(form, T, qkv, expected):
    """the closed form of an edge case on the input the form's reference sees, [64] float64, or None"""
    if expected is None:
        return None
    v = reference_input(form, qkv)[:T, 128:192].astype(np.float64)
    return v.mean(axis=0) if expected == "mean" else v[0]
