"""CPU: the host half of the int8 logits head: wt_quantize_rows_i8 against the numpy restatement,
bit for bit, and wt_tile_rows_i8 through an un-tiler."""
import numpy as np
import pytest

import logits_int8_ref as ref


@pytest.mark.parametrize("K", [128, 384, 512])
def test_quantize_rows_is_bit_equal_to_the_restatement(pkg, K):
    rng = np.random.default_rng(K)
    a = (rng.standard_normal((40, K)) * 10.0 ** rng.uniform(-3, 3, (40, 1))).astype(np.float32)
    a[3] = 0.0                                 # all zero: scale 0, all zeros
    a[5, 7] = -2.0 * np.abs(a[5]).max()        # the largest magnitude is negative: -127, never -128
    s = np.float32(0.125)                      # ties: (j + 0.5) s with mx = 127 s and s a power of two, so a * inv = j + 0.5
    a[6] = 0.0
    a[6, 0], a[6, 1:127] = 127 * s, (np.arange(126) + 0.5) * s
    a[7] = -a[6]
    q, scale = pkg.quantize_rows_i8(a)
    q_ref, scale_ref = ref.quantize_rows(a)
    assert np.array_equal(q, q_ref) and np.array_equal(scale.view(np.uint32), scale_ref.view(np.uint32))
    assert not q[3].any() and scale[3] == 0.0
    assert q[5, 7] == -127 and q.min() == -127
    assert list(q[6, :127]) == [127] + list(range(1, 127)) and np.array_equal(q[7], -q[6])  # away from zero, both signs


@pytest.mark.parametrize("V,K", [(33, 128), (1000, 384)])
def test_tiler_round_trips(pkg, V, K):
    rng = np.random.default_rng(V)
    q = rng.integers(-127, 128, (V, K)).astype(np.int8)
    scale = rng.uniform(0.001, 1.0, V).astype(np.float32)
    tiled, st = pkg.tile_rows_i8(q, scale)
    T = (V + 31) // 32
    # un-tiler: [tile][k / 32][half][lane & 31][16] -> row 32 tile + (lane & 31), column 32 step + 16 half + byte
    rows = tiled.reshape(T, K // 32, 2, 32, 16).transpose(0, 3, 1, 2, 4).reshape(T * 32, K)
    assert np.array_equal(rows[:V], q) and not rows[V:].any()
    assert np.array_equal(st[:V], scale) and not st[V:].any()
