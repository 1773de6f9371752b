"""CPU: the cases, bars and emulation of tests/gemm_ln_ref.py against themselves.
(a) The tile choice: the launchers' own plan functions (wt_dbg_plane_gemm_plan, no GPU work) agree with the restatement in
    gemm_ln_ref.py, every case reaches the fused kernel its table names, and the four small cases of
    test_plane_gemm_with_fused_layernorm that used to return unchecked are the ones that take the 192 x 128 tile.
(b) A plain float32 emulation of the kernels' arithmetic (Emu) stays within ONE QUARTER of every bar of every case: the
    evidence that a correct fp32 kernel can meet them.  EDGE_C is the smallest power of two for which that holds on the edge
    rows.
(c) Emulations with one defect each (DEFECTS) fail: the cases can tell."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_ln_ref as R  # noqa: E402

QUARTER = 0.25


@pytest.fixture(scope="module")
def emu():
    return R.Emu()


# ---------------------------------------------------------------------------------------------------------- (a) ---
def test_plan_functions_agree_with_the_model(pkg):
    for M in (1, 64, 150, 192, 193, 240, 256, 257, 289, 384, 385, 500, 512, 700, 2000, 3000, 48000):
        for n_cu in (0, 1, 2, 8, 11, 224, 256):
            for N, K in ((384, 96), (384, 384), (1152, 384), (256, 64)):
                for epi, planes_out, ln in ((5, False, True), (11, False, True), (5, False, False), (1, True, False), (3, True, False)):
                    p = pkg.plane_gemm_plan(M, N, K, epi, planes_out, ln, n_cu)
                    assert p.mode == 2
                    assert (p.tile, p.schedule, p.fused) == R.plane_plan_model(M, N, K, epi, planes_out, ln, n_cu), (M, n_cu, N, K, epi)
    for M in (1, 129, 193, 384):
        for N in (128, 256, 384, 512, 1536):
            for epi, bf_out, ln, c_rpb, ldc in ((5, False, True, R.CONTIGUOUS, N), (11, False, True, R.CONTIGUOUS, N), (5, False, False, R.CONTIGUOUS, N),
                                                (5, False, True, M - 1 if M > 1 else 1, N), (5, False, True, R.CONTIGUOUS, N + 8),
                                                (1, True, True, R.CONTIGUOUS, N), (1, False, True, R.CONTIGUOUS, N)):
                p = pkg.bf16_gemm_plan(M, N, epi, bf_out, ln, c_rpb, ldc)
                want = R.bf16_plan_model(M, N, epi, bf_out, ln, c_rpb, ldc)
                assert (p.bn, p.bm, p.whole_row) == want, (M, N, epi, bf_out, ln, c_rpb, ldc)


def test_every_case_reaches_the_kernel_its_table_names(pkg):
    for tile, M, n_cu in R.PLANE_TABLE:
        for K in R.PLANE_KS:
            for epi, _ in R.EPILOGUES:
                p = pkg.plane_gemm_plan(M, 384, K, epi, False, True, n_cu)
                assert (p.tile, p.schedule, p.fused) == (tile, 2 if tile == 1 else 0, True), (tile, M, n_cu, p.kernel)
    for family, N, M, n_cu in R.FLAG_SHAPES + R.REPEAT_SHAPES:
        bm, _, _ = R.geometry(family, M, N, 64, 5, n_cu)
        if family == 0:
            assert pkg.plane_gemm_plan(M, N, 64, 5, False, True, n_cu).fused
        else:
            assert pkg.bf16_gemm_plan(M, N, 5, False, True).whole_row
    for family, N, M, n_cu in R.FLAG_SHAPES:
        bm = R.geometry(family, M, N, 64, 5, n_cu)[0]
        assert (M - 1) % bm == bm // 2, "row M - 1 must be alone in the second wavefront row of the last tile"
    for family, N, M, n_cu in R.REPEAT_SHAPES:
        bm = R.geometry(family, M, N, 64, 5, n_cu)[0]
        assert (M - 1) % bm == (128 if bm == 256 else 0), "the last tile (256 rows: its second wavefront row) must hold one row"
    assert {R.geometry(0, M, 384, 64, 5, n)[0] for f, N, M, n in R.REPEAT_SHAPES if f == 0} == {192, 256}
    # the gap as found: these cases of test_plane_gemm_with_fused_layernorm take the narrow tile and fuse nothing
    for M, K, epi, n_cu in ((500, 384, 5, 0), (700, 1536, 5, 224), (3000, 96, 11, 0), (193, 384, 5, 0)):
        p = pkg.plane_gemm_plan(M, 384, K, epi, False, True, n_cu)
        assert (p.tile, p.fused) == (0, False)
    for n_cu, tile in ((224, 2), (256, 1)):
        p = pkg.plane_gemm_plan(48000, 384, 384, 5, False, True, n_cu)
        assert (p.tile, p.fused) == (tile, True)


# ---------------------------------------------------------------------------------------------------------- (b) ---
def test_emulation_stays_under_a_quarter_of_every_bar(emu):
    worst = {}
    cases = R.all_cases()
    for i, c in enumerate(cases):
        res, _ = R.run_case(emu, c, QUARTER, without_y32=i % 9 == 0, scales=R.LN_SCALES if i % 9 == 0 else ())
        for k, v in res.items():
            key = ("bf16 " if c.family else "planes ") + k
            worst[key] = max(worst.get(key, 0.0), v)
    print({k: round(v, 4) for k, v in worst.items()})
    assert len(cases) == 9 * 9 + 2 + 3 * 12
    assert {(c.family, c.bm, c.N) for c in cases} == {(0, 192, 384), (0, 256, 384), (1, 192, 128), (1, 192, 384), (1, 128, 512)}


@pytest.mark.parametrize("family", [0, 1], ids=["planes", "bf16"])
def test_emulation_on_the_edge_rows(emu, family):
    for c in [R.edge_case(family)] + ([R.edge_case(0, 385, 1)] if family == 0 else []):
        assert set(c.edge.values()) == set(R.EDGE_KINDS)
        regions = {(r // c.bm, r % c.bm >= c.bm // 2) for r in c.edge}
        assert len(regions) == 4, "both tiles and both wavefront rows"
        R.run_case(emu, c, QUARTER, scales=R.LN_SCALES)


def test_edge_c_is_the_smallest_power_of_two():
    assert R.derive_edge_c() == R.EDGE_C


def test_flag_cases_on_the_emulation(emu):
    for shape in R.FLAG_SHAPES:
        R.flag_checks(emu, *shape)


# ---------------------------------------------------------------------------------------------------------- (c) ---
def run_everything(backend):
    for family in (0, 1):
        R.run_case(backend, R.edge_case(family), scales=R.LN_SCALES)
    for c in R.plane_cases(1, 193, 2)[:3] + R.plane_cases(2, 385, 1)[:3] + R.bf16_cases(512)[4:6]:
        R.run_case(backend, c)
    for shape in R.FLAG_SHAPES:
        R.flag_checks(backend, *shape)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defective_emulations_fail(defect):
    """at the FULL bars (margin 1), on a subset of what the GPU test runs"""
    with pytest.raises(AssertionError) as ei:
        run_everything(R.Emu(defect))
    print(defect, "->", str(ei.value)[:200])


def test_the_subset_passes_on_the_correct_emulation(emu):
    run_everything(emu)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_is_caught_in_both_families_where_it_applies(defect):
    """the bf16 family has no ln_scale; every other defect must show in each family on its own"""
    for family in (0, 1):
        if defect == "scale_on_lo_only" and family == 1:
            continue
        with pytest.raises(AssertionError):
            R.run_case(R.Emu(defect), R.edge_case(family), scales=R.LN_SCALES)
            for shape in R.FLAG_SHAPES:
                if shape[0] == family:
                    R.flag_checks(R.Emu(defect), *shape)
