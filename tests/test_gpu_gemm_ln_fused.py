"""GPU (-m gpu): the encoder GEMMs' fused LayerNorm epilogue (planes_epilogue<..., LN = true> in k_gemm_planes.hip,
bf16_epilogue<..., LN> in k_gemm_bf16.hip) at ragged tiles and edge rows, through the tap wt_dbg_gemm_ln_fused, which puts
256 guard rows behind every output.  Cases, float64 reference, bars and every assertion live in tests/gemm_ln_ref.py
(DESIGN section 26); tests/test_gemm_ln_reference.py shows on the CPU that a float32 emulation meets a quarter of each bar
and that five defective emulations do not meet them.

Every case first asserts what the launcher's own plan function (wt_dbg_plane_gemm_plan) says it will launch, then that the
launch reported the fusion: a case that reaches another kernel fails, it does not return.  Every case prints the kernel it
reached and its measured errors as fractions of their bars."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_ln_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SCHEDULE_OF_MODE = {2: 2, 1: 1, 0: 0}   # wt_dbg_set_plane_gemm_mode -> schedule of the 192 x 384 tile (pp16, pp, in step)


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


class plane_mode:
    """the schedule of the 192 x 384 tile for the launches inside; the default (2) is restored on the way out"""

    def __init__(self, pkg, mode):
        self.L, self.mode = pkg.lib(), mode

    def __enter__(self):
        assert self.L.wt_dbg_set_plane_gemm_mode(self.mode) == 0

    def __exit__(self, *exc):
        assert self.L.wt_dbg_set_plane_gemm_mode(2) == 0


def assert_plan(pkg, c, mode=2):
    """the launcher's own word on what it will launch for the case; returns the kernel's name"""
    if c.family == 0:
        p = pkg.plane_gemm_plan(c.M, c.N, c.K, c.epi, False, True, c.n_cu)
        tile = 1 if c.bm == 192 else 2
        want = (tile, SCHEDULE_OF_MODE[mode] if tile == 1 else 0, True, mode)
        assert (p.tile, p.schedule, p.fused, p.mode) == want, (c.name, p.kernel)
    else:
        p = pkg.bf16_gemm_plan(c.M, c.N, c.epi, False, True)
        assert (p.bn, p.bm, p.whole_row) == (c.N, c.bm, True), (c.name, p.kernel)
    return p.kernel


TABLE = [pytest.param(tile, M, n_cu, mode, id=f"{R.TILE_NAMES[tile]}-M{M}-cu{n_cu}-mode{mode}")
         for tile, M, n_cu in R.PLANE_TABLE for mode in ((2, 1, 0) if tile == 1 else (2,))]


@pytest.mark.parametrize("tile,M,n_cu,mode", TABLE)
def test_plane_gemm_fused_layernorm(pkg, eng, tile, M, n_cu, mode):
    """K = 32, 96, 384 x epilogue 5 in place, 11 with pos_period 32 and 100, at every edge of the table; the 192-row tile under
    each of its three schedules.  ln_scale goes round 1, 64, 1024; the first case also runs every scale and without ln_y32."""
    with plane_mode(pkg, mode):
        for i, c in enumerate(R.plane_cases(tile, M, n_cu)):
            kernel = assert_plan(pkg, c, mode)
            R.run_case(eng, c, without_y32=i == 0, scales=R.LN_SCALES if i == 0 else (), kernel=kernel)


@pytest.mark.parametrize("M,n_cu", [(M, n) for tile, M, n in R.PLANE_TABLE if tile == 1])
def test_in_step_and_ping_pong_give_the_same_bits(pkg, eng, M, n_cu):
    """gemm_planes_tile<..., 3, LN> and gemm_planes_pp<..., LN> run the same MFMA shape in the same order: every output word
    agrees (test_plane_gemm_every_tile_shape_gives_the_same_result claims it for the plain epilogue)."""
    for epi, period in R.EPILOGUES[:2]:
        c = R.make_case(0, 384, M, 96, epi, n_cu, period)
        outs = []
        for mode in (0, 1):
            with plane_mode(pkg, mode):
                print(c.name, "->", assert_plan(pkg, c, mode))
                outs.append(R.launch(eng, c)[1])
        for what in ("C", "planes", "y32"):
            assert np.array_equal(R.bits(getattr(outs[0], what)), R.bits(getattr(outs[1], what))), (c.name, what)
        assert outs[0].fused and outs[1].fused and outs[0].flag == outs[1].flag == 0


@pytest.mark.parametrize("family", [0, 1], ids=["planes", "bf16"])
def test_conv2_form_with_fused_layernorm(pkg, eng, family):
    """epilogue 11 over conv2's overlapping stride-2 rows, three clips of T = 100: clip boundaries inside 32-row slabs"""
    c = R.conv2_case(family)
    R.run_case(eng, c, without_y32=True, kernel=assert_plan(pkg, c))


@pytest.mark.parametrize("N", sorted(R.BF16_ROWS))
def test_bf16_gemm_fused_layernorm(pkg, eng, N):
    """the three whole-row tiles at M = 1, one tile plus one row and two whole tiles, K = 64 and 192, both epilogues (the
    epilogue-11 instantiations are launched by no other kernel test)"""
    for i, c in enumerate(R.bf16_cases(N)):
        R.run_case(eng, c, without_y32=i < 2, kernel=assert_plan(pkg, c))


@pytest.mark.parametrize("family,M,n_cu", [(0, 289, 1), (0, 385, 1), (1, 289, 0)], ids=["planes-192", "planes-256", "bf16"])
def test_edge_rows(pkg, eng, family, M, n_cu):
    """constant rows (ln_b bit for bit), mean 1e4 at spread 1, spread 1e-3, magnitudes 1e-6 .. 1e3, zero gains and shifts,
    in both tiles and both wavefront rows; the planes at every ln_scale"""
    c = R.edge_case(family, M, n_cu)
    res, _ = R.run_case(eng, c, without_y32=True, scales=R.LN_SCALES, kernel=assert_plan(pkg, c))
    assert "edge" in res


@pytest.mark.parametrize("family,N,M,n_cu", R.FLAG_SHAPES)
def test_nonfinite_flag(pkg, eng, family, N, M, n_cu):
    c = R.make_case(family, N, M, 64, R.EPI_RESIDUAL, n_cu)
    print(f"flag family {family} N {N} M {M}:", assert_plan(pkg, c), R.flag_checks(eng, family, N, M, n_cu))


def base_case(family):
    return R.make_case(family, 384, 193, 64, R.EPI_RESIDUAL, 2 if family == 0 else 0, seed=11)


def buffers(c):
    C = np.full((c.M + R.GUARD, c.N), np.nan, np.float32)
    C[:c.M] = c.R
    return C, (c.fills.bf if c.family else c.fills.f16).copy(), c.fills.f32.copy()


REFUSALS = {
    "no-gain": dict(ln_g=None),
    "no-shift": dict(ln_b=None),
    "ln_scale=0": dict(ln_scale=0.0),
    "ln_scale<0": dict(ln_scale=-64.0),
    "ldc!=N": dict(ldc=392),
    "c_rpb<M": dict(c_rpb=192, c_bs=192 * 384),
    "plane-output-too": dict(p_out=True),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_plane_gemm_refuses_what_the_fusion_cannot_take(pkg, eng, name):
    """WT_ERR_INVALID_ARG from launch_gemm_planes before anything is launched; every output as given"""
    c = base_case(0)
    C, planes, y32 = buffers(c)
    before = [C.copy(), planes.copy(), y32.copy()]
    over = dict(REFUSALS[name])
    if over.get("p_out"):
        over["p_out"] = np.zeros_like(planes)
    a = dict(M=c.M, N=c.N, K=c.K, A=c.A, a_rpb=c.a_rpb, a_bs=c.a_bs, lda=c.lda, W=c.W, bias=c.bias, C=C, planes=planes, ln_g=c.g,
             ln_b=c.b, ln_scale=64.0, y32=y32, n_cu=c.n_cu, copy=False)
    a.update(over)
    with pytest.raises(pkg.WtError) as ei:
        eng.dbg_gemm_ln_fused(0, c.epi, **a)
    assert ei.value.code == 1, name
    for got, was in zip((C, planes, y32), before):
        assert np.array_equal(R.bits(got), R.bits(was)), name
    a.update(dict(ln_g=c.g, ln_b=c.b, ln_scale=64.0, ldc=384, c_rpb=R.CONTIGUOUS, c_bs=0, p_out=None))  # the valid launch they depart from
    assert eng.dbg_gemm_ln_fused(0, c.epi, **a).fused


BF16_UNFUSED = {
    "no-gain": (384, dict(ln_g=None)),
    "no-shift": (384, dict(ln_b=None)),
    "ldc!=N": (384, dict(ldc=392)),
    "c_rpb<M": (384, dict(c_rpb=192, c_bs=192 * 384)),
    "N=256": (256, dict()),
}


@pytest.mark.parametrize("name", sorted(BF16_UNFUSED))
def test_bf16_gemm_falls_back_to_the_plain_tile(pkg, eng, name):
    """the conditions of bf16_gemm_plan: fused == False, the LayerNorm outputs as given, and the plain result still right"""
    N, over = BF16_UNFUSED[name]
    c = R.make_case(1, N, 193, 64, R.EPI_RESIDUAL, seed=11, fusable=N != 256)
    ldc = over.get("ldc", N)
    p = pkg.bf16_gemm_plan(c.M, N, c.epi, False, over.get("ln_g", 1) is not None and over.get("ln_b", 1) is not None,
                           over.get("c_rpb", R.CONTIGUOUS), ldc)
    assert not p.whole_row, name
    C0 = np.full((c.M + R.GUARD) * N, np.nan, np.float32)
    idx = (np.arange(c.M) * ldc)[:, None] + np.arange(N)[None, :]
    C0[idx] = c.R
    C0 = C0.reshape(-1, N)
    _, out = R.launch(eng, c, C=C0, **over)
    assert not out.fused and out.flag == 0, name
    assert np.array_equal(out.planes, c.fills.bf) and np.array_equal(R.bits(out.y32), R.bits(c.fills.f32)), name
    ref = R.reference(c)[0]
    got = out.C.reshape(-1)[idx].astype(np.float64)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{name}: {p.kernel}: C {err / R.C_BAR:.3g} of its bar")
    assert err < R.C_BAR
    keep = np.ones(C0.size, bool)
    keep[idx.ravel()] = False
    assert np.array_equal(R.bits(out.C.reshape(-1)[keep]), R.bits(C0.reshape(-1)[keep])), name + ": a cell outside the launch's own was written"


REPEATS = [pytest.param(f, N, M, n, mode, id=f"{'bf16' if f else 'planes'}-N{N}-M{M}-mode{mode}")
           for f, N, M, n in R.REPEAT_SHAPES for mode in ((2, 1, 0) if (f, M) == (0, 193) else (2,))]


@pytest.mark.parametrize("family,N,M,n_cu,mode", REPEATS)
def test_same_bits_every_call(pkg, eng, family, N, M, n_cu, mode):
    """six runs of each fused kernel at its one-row-last-tile shape, each behind a call of the same shape on huge values:
    the first call's bits every time (nothing left in LDS or registers by the call before reaches a result)"""
    c = R.make_case(family, N, M, 64, R.EPI_RESIDUAL, n_cu, seed=5)
    huge = R.make_case(family, N, M, 64, R.EPI_RESIDUAL, n_cu, seed=6)
    huge.A, huge.R, huge.bias = huge.A * np.float32(1e3), huge.R * np.float32(1e20), huge.bias * np.float32(1e10)
    with plane_mode(pkg, mode):
        print(c.name, "->", assert_plan(pkg, c, mode))
        C0, first = R.launch(eng, c)
        R.check(c, C0, first)
        for _ in range(6):
            assert R.launch(eng, huge)[1].fused
            again = R.launch(eng, c)[1]
            for what in ("C", "planes", "y32"):
                assert np.array_equal(R.bits(getattr(again, what)), R.bits(getattr(first, what))), (c.name, what)
            assert again.fused and again.flag == 0
