"""No GPU: the inputs, references and bars of tests/test_gpu_encoder_attention.py (tests/attn_cases.py) on their own.  A
plain numpy float32 attention must meet every tolerance of groups a, b and d for the chosen inputs, else a bar would ask
of the kernels what fp32 arithmetic cannot give; and the closed forms of the edge cases must agree with the float64
softmax they stand next to."""
import numpy as np
import pytest

import attn_cases as ac


def test_f16_scale_for_is_the_largest_power_of_two_under_the_bound():
    # (the last six: bounds whose quotient 16384 / bound overflows float32, subnormal ones, and the largest finite ones)
    for bound in (1e-9, 2.0 ** -11, 0.3, 1.0, 4.4, 16384.0, 16385.0, 3e4, 1e12, 4.8e-35, 1e-38, 2.0 ** -140, 2.0 ** -149, 2.0 ** 127,
                  3.4e38):
        s = ac.f16_scale_for(bound)
        assert np.log2(s) == round(np.log2(s)) and 2.0 ** -24 <= s <= 2.0 ** 24
        assert s == 2.0 ** -24 or bound * s <= 16384.0
        assert s == 2.0 ** 24 or bound * 2 * s > 16384.0
    assert ac.f16_scale_for(0.0) == 1.0 and ac.f16_scale_for(float("nan")) == 1.0 and ac.f16_scale_for(-1.0) == 1.0
    assert ac.f16_scale_for(float("inf")) == 2.0 ** -24 and ac.f16_scale_for(1e-36) == 2.0 ** 24


def test_sweep_reaches_every_grid_residue_and_tile_edge():
    assert {g & 7 for _, _, _, g in ac.SWEEP} == set(range(8))
    assert all(B * H * ((T + 127) // 128) == g for B, T, H, g in ac.SWEEP)
    lengths = {T for _, T, _, _ in ac.SWEEP}
    assert {1, 63, 65, 127, 128, 129, 193, 257} <= lengths


@pytest.mark.parametrize("B,T,H,grid", ac.SWEEP)
def test_float32_attention_meets_the_sweep_bars(B, T, H, grid):
    qkv, refs = ac.normal_case(B, T, H)
    for form in ac.FORMS:
        x, ref = refs[form == "bf16"]
        ac.check_against(form, ac.attention(x, B, T, H, np.float32), ref, x, B, T, H, f"a ({B}, {T}, {H})")


@pytest.mark.parametrize("case", list(ac.SCALE_CASES))
@pytest.mark.parametrize("B,T,H", ac.SCALE_SHAPES)
def test_float32_attention_meets_the_scale_bars(B, T, H, case):
    j, log2_v = ac.SCALE_CASES[case]
    qkv, ref = ac.scale_case(B, T, H, log2_v)
    scales = ac.plane_scales(qkv, B, T, H, j)
    m = ac.data_maxima(qkv, B, T, H)
    for i in range(3):  # the scaled operands stay a factor 2^j..2^(j+1) under 16384, inside fp16
        assert 16384.0 / 2.0 ** (j[i] + 1) < m[i] * scales[i] <= 16384.0 / 2.0 ** j[i]
    ac.check_against("planes", ac.attention(qkv, B, T, H, np.float32), ref, qkv, B, T, H, f"b {case}")


@pytest.mark.parametrize("case", ac.EDGE_CASES)
def test_edge_cases_in_float32_and_their_closed_forms(case):
    T, qkv, expected = ac.edge_case(case)
    for form in ac.FORMS:
        x = ac.reference_input(form, qkv)
        ref = ac.attention(x, 1, T, 1)
        ac.check_against(form, ac.attention(x, 1, T, 1, np.float32), ref, x, 1, T, 1, f"d {case}")
        want = ac.edge_expected(form, T, qkv, expected)
        if want is not None:
            assert np.abs(ref - want).max() < 1e-13 * max(1.0, np.abs(want).max()), form
    if case.startswith("dominant"):  # the dominating key takes all but e^-30 of every row
        q, k, _ = ac.thirds(qkv, 1, T, 1, np.float64)
        s = (q[0, :, 0] @ k[0, :, 0].T) / 8.0
        j_star = int(case.split("-k")[1])
        assert (s.argmax(-1) == j_star).all() and (np.sort(s, -1)[:, -1] - np.sort(s, -1)[:, -2] > 30).all()
    if case == "falling-ramp":  # 9 log2 units per 64-key tile, within the noise of the 0.05 perturbation
        q, k, _ = ac.thirds(qkv, 1, T, 1, np.float64)
        s = (q[0, :, 0] @ k[0, :, 0].T) / 8.0 * 1.4426950408889634
        assert np.abs((s[:, 64:] - s[:, :-64]).mean() + 9.0) < 0.2
