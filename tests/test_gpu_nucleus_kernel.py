"""GPU (-m gpu): nucleus_cut (csrc/k_nucleus.hip) through wt_dbg_nucleus_cut against
tests/nucleus_ref.py: cut and kept EQUAL, kept_q / total_q within 1e-5 of the mass ratio.  The kernel forms p in fp32
(exp2 of one fma, floored at 2^-40: under 1e-6 relative), so every top-p case has room at its boundary: the mass of N, and
of N without its last id, lie at least 1e-4 of the mass of K from the target.  That is asserted for every case; the seeds
were chosen on the CPU so that it holds.  Rows are peaked as a decoder's are (a head of a few ids over a body 30 below),
so a top-p boundary falls on an id with real mass; top-k boundaries fall into the body, where the count decides."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucleus_ref as nr  # noqa: E402

pytestmark = pytest.mark.gpu
SB, ONE, TEMPS = 2, np.ones(1, np.float32), np.array([0.8, 0.5, 1.0], np.float32)
# test_sizes: per (V, rows) the first seed whose rows keep 4e-4 of room in every top-p case
SEEDS = {(5, 1): 1, (5, 3): 2, (4096, 1): 1, (4096, 3): 2, (4097, 1): 4, (4097, 3): 13, (51865, 1): 6, (51865, 3): 12,
         (65536, 1): 1, (65536, 3): 1, (65540, 1): 2, (65540, 3): 2}


@pytest.fixture(scope="module")
def eng(pkg, assets):
    e = pkg.Engine(*assets("micro"), True)
    yield e
    e.close()


def peaked(seed, rows, V, head=12, step=1.1):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((rows, V)) * 2.0 - 30.0).astype(np.float32)
    for r in range(rows):
        ids = rng.choice(V, min(head, V - 1), replace=False)
        z[r, ids] = -np.cumsum(rng.uniform(0.5 * step, 1.5 * step, ids.size)).astype(np.float32)
    return z


def check(eng, z, top_k, top_p, temps=TEMPS, gens=(), ts=False, eot=0, beg=1):
    z = np.ascontiguousarray(z, np.float32)
    temps = np.resize(temps, z.shape[0])
    ids = np.ones((z.shape[0], SB + len(gens) + 1), np.int64)
    ids[:, SB:SB + len(gens)] = gens
    got = eng.dbg_nucleus_cut(z, ids, SB + len(gens), SB, temps, top_k, top_p, ts, eot, beg)
    for r in range(z.shape[0]):
        ref = nr.cut(z[r], nr.rule_mask(z[r], gens, eot, beg, 50, ts), temps[r], top_k, top_p)
        ratio = int(got["kept_q"][r]) / int(got["total_q"][r])
        print(f"V={z.shape[1]} k={top_k} p={top_p} row {r}: kept {ref['kept']} margin {ref['margin']:.3g} ratio {ref['ratio']:.7f} / {ratio:.7f}")
        assert ref["margin"] >= 1e-4, (r, ref["margin"])  # a condition on the inputs, never a skip
        assert (int(got["cut"][r]), int(got["kept"][r])) == (ref["cut"], ref["kept"]), (r, got[r])
        assert abs(ratio - ref["ratio"]) <= 1e-5
    return got


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("V", [5, 4096, 4097, 51865, 65536, 65540])
def test_sizes_top_k_top_p(eng, V, rows):
    """One quad, the sampler's chunk edge, a Whisper row, the last size in registers and the first that is re-read."""
    z = peaked(SEEDS[V, rows], rows, V)
    for k, p in [(k, 1.0) for k in (1, 2, 50, V, V + 7)] + [(0, p) for p in (0.001, 0.5, 0.9, 0.999)] + [(50, 0.9)]:
        check(eng, z, k, p)


def test_top_p_over_the_renormalised_top_k(eng):
    """120 ids of slowly falling mass: 0.9 of the top-50 mass ends inside the top 50, 0.9 of the whole beyond them."""
    z = peaked(6, 3, 51865, head=120, step=0.02)
    assert (check(eng, z, 50, 0.9)["kept"] < 50).all() and (check(eng, z, 0, 0.9)["kept"] > 50).all()


def test_ties_and_equal_rows(eng):
    """Four equal logits across the k-cut and the p-cut: the larger ids stay.  A row of equal logits: ids decide."""
    V = 4097
    z = np.full((1, V), -30.0, np.float32)
    z[0, [4000, 7, 4096, 90, 2500, 33]] = [0.0, -1.0, -1.0, -1.0, -1.0, -3.0]
    assert int(check(eng, z, 3, 1.0, ONE)["cut"][0]) & 0xffffffff == 2500
    got = check(eng, z, 0, 0.7, ONE)  # 1 + 3 e^-1 of 2.52 reaches 0.7, 1 + 2 e^-1 does not
    assert int(got["kept"][0]) == 4 and int(got["cut"][0]) & 0xffffffff == 90
    for k, p in ((10, 1.0), (0, 0.5), (V - 1, 1.0), (1000, 0.2505)):
        got = check(eng, np.full((1, V), 1.5, np.float32), k, p, ONE)
    assert int(got["kept"][0]) == 251 and int(got["cut"][0]) & 0xffffffff == V - 251


@pytest.mark.parametrize("shift", [0, 10, 21])
def test_each_radix_level_decides(eng, shift):
    """Logits that differ only in the low ten bits of the float, the next eleven, or the top eleven (with many ties)."""
    V, rng = 4097, np.random.default_rng(shift)
    if shift == 21:  # sign, exponent and two mantissa bits: +-{1, 1.25, 1.5, 1.75} 2^e, e = -2 .. 2
        z = rng.choice(np.array([s * f * 2.0 ** e for s in (1, -1) for f in (1, 1.25, 1.5, 1.75) for e in range(-2, 3)], np.float32), (2, V))
    else:
        z = (np.uint32(0x40000000) + (rng.integers(0, 1 << (10 if shift == 0 else 11), (2, V)).astype(np.uint32) << np.uint32(shift))).view(np.float32)
    for k, p in [(1, 1.0), (50, 1.0), (2049, 1.0), (V - 1, 1.0)] + ([(0, 0.3), (700, 0.6)] if shift == 21 else []):
        check(eng, z, k, p)


@pytest.mark.parametrize("V", [4097, 51865])
def test_restricted_to_the_timestamp_rules(eng, V):
    """A = a text and a timestamp range from a TsState, -inf inside both; larger logits outside A must not count."""
    rng = np.random.default_rng(V)
    beg = V - 1501 if V > 8192 else V - 101
    eot = beg - 107 if V > 8192 else beg - 7
    z = peaked(V, 3, V)
    z[:, eot + 1:beg], z[:, beg:beg + 4] = 5.0, 7.0  # rule 1; below the last timestamp (rule 3)
    z[:, rng.integers(0, V, V // 4)] = -np.inf
    gens = [beg + 3, 17]  # text, or timestamps from tick 4 on
    z[:, [11, 300, beg + 9, beg + 40, eot]] = [0.0, -0.8, -1.9, -2.7, -3.9]
    for k, p in ((1, 1.0), (3, 1.0), (50, 1.0), (0, 0.5), (0, 0.9), (0, 0.999), (4, 0.9)):
        check(eng, z, k, p, gens=gens, ts=True, eot=eot, beg=beg)
    z[:, beg + 4:] = -np.inf  # suppression left no timestamp
    check(eng, z, 2, 0.9, gens=gens, ts=True, eot=eot, beg=beg)

