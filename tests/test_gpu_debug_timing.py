"""GPU (-m gpu): the timed branch (iters > 0) of the debug taps that can time their kernel (include/wt_debug.h).
Every other test calls them with iters = 0.  A timed call must succeed, return a finite positive time, and leave the
data it returns exactly what the untimed call returns; nothing is asserted about how long a launch takes.  Shapes are
the smallest ones of each tap's own correctness test (tests/test_gpu_kernels.py)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 2


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def check_time(t):
    assert math.isfinite(t) and t > 0.0, t


def gemm_operands(M=1, N=128, K=64):
    rng = np.random.default_rng(M + 3 * N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    return A, W, rng.standard_normal(N).astype(np.float32)


def test_gemm_planes_timed(eng):
    A, W, bias = gemm_operands()
    C, ms = eng.dbg_gemm_planes(A, W, bias, epi=1, iters=ITERS)
    check_time(ms)
    assert np.array_equal(C, eng.dbg_gemm_planes(A, W, bias, epi=1))


def test_gemm_bf16_timed(eng):
    A, W, bias = gemm_operands()
    C, ms = eng.dbg_gemm_bf16(A, W, bias, epi=1, iters=ITERS)
    check_time(ms)
    assert np.array_equal(C, eng.dbg_gemm_bf16(A, W, bias, epi=1))


@pytest.mark.parametrize("tap", ["dbg_encoder_attention_planes", "dbg_encoder_attention_bf16"])
def test_encoder_attention_timed(eng, tap):
    B, T, H = 1, 64, 1
    qkv = np.random.default_rng(B * 1000 + T + H).standard_normal((B * T, 3 * 64 * H)).astype(np.float32)
    out, ms = getattr(eng, tap)(qkv, B, T, H, iters=ITERS)
    check_time(ms)
    assert np.array_equal(out, getattr(eng, tap)(qkv, B, T, H))


@pytest.mark.parametrize("bf16", [False, True])
def test_cross_absorbed_timed(eng, bf16):
    B, H, T, chunks, nq = 2, 2, 100, 2, 4
    rng = np.random.default_rng(B * 1000 + T + H + nq)
    d = 64 * H
    E = rng.standard_normal((B, T, d)).astype(np.float32)
    qp = (rng.standard_normal((nq * B, H * d)) * (3.0 / np.sqrt(d))).astype(np.float32)
    wv = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    bv = rng.standard_normal(d).astype(np.float32)
    out, us = eng.dbg_cross_absorbed(qp, E, wv, bv, B, H, T, chunks, nq, iters=ITERS, bf16=bf16)
    check_time(us)
    assert np.array_equal(out, eng.dbg_cross_absorbed(qp, E, wv, bv, B, H, T, chunks, nq, bf16=bf16))


def test_gemm_bench(eng):
    check_time(eng.dbg_gemm_bench(1, 128, 64, epi=1, variant=0, iters=ITERS))


# kind 0: residual GEMM, 1: LayerNorm + GEMM, 2: combine + residual GEMM, 3: LayerNorm + logits + argmax records
@pytest.mark.parametrize("kind,N,K", [(0, 128, 128), (1, 384, 128), (2, 128, 128), (3, 1000, 128)])
def test_dec_gemm_bench(eng, kind, N, K):
    check_time(eng.dbg_dec_gemm_bench(kind, 2, N, K, rows=4, iters=ITERS))
