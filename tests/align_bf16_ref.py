"""Reference for the bf16 form of align_scores (k_align.hip): the cases the kernel test runs, the
float64 weights on the bf16-rounded operands, and a float32 emulation of the kernel's score product.

The kernel rounds q' to bf16 in registers (to nearest even), reads E as ONE bf16 plane and runs one
v_mfma_f32_16x16x32_bf16 per 32 columns with fp32 accumulation: a bf16 x bf16 product has 16 significant bits and is
exact in fp32, so the only error of a score is the fp32 accumulation's.  The emulation restates that on numpy: exact
fp32 products, the 32 products of a step added in fp32, the steps added to an fp32 accumulator in ascending order.
tests/test_full_bf16_all_reference.py holds it to a quarter of the kernel test's bar on the kernel test's own shapes."""
import numpy as np

from decoder_attn_ref import bf16_round

W_BOUND = 1e-4  # the bar of tests/test_gpu_align_kernels.py: |W - W64| / W64 over the weights above 1e-30
T_SHORT, T_LONG = 100, 1500  # six 16-frame tiles and 4 frames; 94 tiles, the last of 12 frames

# (H, B, pos0, n_pos) at T_SHORT: the fp32 kernel test's shapes and one d_model = 512
SHAPES = [(2, 1, 0, 1), (2, 3, 2, 5), (6, 3, 2, 5), (2, 32, 0, 4), (6, 32, 0, 4), (2, 1, 96, 32), (8, 3, 2, 5)]
LONG_SHAPE = (6, 2, 0, 32)  # at T_LONG, F = (1500, 205)


def case(H, B, T, n_pos, seed, spread=13.0):
    """Queries fp32 [n_pos][B][H * d] and E [B][T][d] of bf16 values whose scores have a standard deviation of `spread`
    log2 units (+-40 at three sigma), as tests/test_gpu_align_kernels.py draws them."""
    rng = np.random.default_rng(seed)
    d = 64 * H
    E = bf16_round(rng.standard_normal((B, T, d)).astype(np.float32)).reshape(B, T, d)
    qp = (rng.standard_normal((n_pos, B, H * d)) * (spread / np.sqrt(d))).astype(np.float32)
    return qp, E


def seed_of(H, B, n_pos, T):
    return 7000 + 1000 * H + 10 * B + n_pos + T


def frames(B, T):
    """F_b among 1, T and values that are multiples of neither 4 nor 16, mixed inside the batch"""
    return np.array([(1, 3, 37, T)[(b + B) % 4] for b in range(B)], np.int32)


def softmax2(S, F):
    """S [..., T] log2-domain scores -> float64 weights over t < F, zero behind."""
    S = np.asarray(S, np.float64)
    W = np.zeros_like(S)
    x = S[..., :F]
    x = np.exp2(x - x.max(axis=-1, keepdims=True))
    W[..., :F] = x / x.sum(axis=-1, keepdims=True)
    return W


def rounded_query(qp, b, h, d):
    return bf16_round(np.ascontiguousarray(qp[:, b, h * d:(h + 1) * d])).reshape(qp.shape[0], d)


def scores64(qp, E, b, h):
    """float64 scores [n_pos][T] of head h of clip b on the bf16-rounded operands"""
    d = E.shape[2]
    return np.einsum("pd,td->pt", rounded_query(qp, b, h, d).astype(np.float64), bf16_round(E[b]).reshape(E[b].shape).astype(np.float64))


def scores_emulated(qp, E, b, h):
    """The kernel's arithmetic in float32: rounded operands, exact products, fp32 accumulation in steps of 32 columns."""
    d = E.shape[2]
    q = rounded_query(qp, b, h, d)
    e = bf16_round(E[b]).reshape(E[b].shape)
    acc = np.zeros((q.shape[0], e.shape[0]), np.float32)
    for c in range(0, d, 32):
        prod = q[:, None, c:c + 32] * e[None, :, c:c + 32]  # float32, exact
        acc = (acc + prod.sum(axis=-1, dtype=np.float32)).astype(np.float32)
    return acc


def relative_error(got, want):
    """largest |got - want| / want over want > 1e-30, and the largest got elsewhere"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    big = want > 1e-30
    rel = float((np.abs(got - want)[big] / want[big]).max()) if big.any() else 0.0
    small = float(got[~big].max()) if (~big).any() else 0.0
    return rel, small
