"""GPU (-m gpu): the absorbed cross-attention on an int8 image of the encoder output (k_cross_absorbed_i8.hip, option
cross_int8) through the chain tap wt_dbg_cross_absorbed_i8_chain, against cross_int8_ref.

Inputs as test_gpu_cross_absorbed.py draws them.  The int8 image and its scales equal the numpy quantiser bit for bit;
behind the quantisers all is fp32-level arithmetic, so the output is held to the fp16-plane form's 2e-5 against the
float64 reference on the DEQUANTISED operands, which lies more than 100 bars from the unquantised one."""
import numpy as np
import pytest

import cross_int8_ref as ref
from test_gpu_cross_absorbed import M_EMPTY, OUT_FILL, WS_FILL, draw, eng, groups, n_nonempty, reference  # noqa: F401 (eng: fixture)

pytestmark = pytest.mark.gpu
BAR = 2e-5

CASES = [
    (7, 6, 3, 97, 3, 2),     # d 384: three sources, the last of one clip; the third chunk is empty; 12 query columns
    (7, 8, 2, 97, 3, 2),     # d 512: four sources, a shorter last one; 16 query columns
    (5, 2, 4, 70, 4, 3),     # d 128: two sources; three tiles in four chunks
    (6, 8, 3, 130, 2, 1),    # two sources; chunks of three and two tiles, the last one ragged
    (64, 6, 32, 33, 2, 1),   # 64 = 2 x 32 clips; one key in the second chunk
    (3, 2, None, 70, 1, 8),  # one source; 16 query columns at d 128
    (2, 6, None, 230, 1, 2), # eight tiles in one chunk: the ring of four stages wraps
]


@pytest.mark.parametrize("bf16", [False, True], ids=["planes", "bf16"])
@pytest.mark.parametrize("B,H,split,T,chunks,nq", CASES)
def test_against_the_quantised_float64_reference(eng, B, H, split, T, chunks, nq, bf16):
    d = 64 * H
    rng = np.random.default_rng(B * 131 + H * 17 + T + chunks + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    E[0, 5] = 0.0                                            # an all-zero key row: zeros with scale 0
    srcs = groups(E, split) if split else [E]
    out, ws, qe, se, e_scale = eng.dbg_cross_absorbed_i8_chain(qp, srcs, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16)
    assert (out[-1] == OUT_FILL).all() and (ws[-1] == WS_FILL).all(), "a guard row was written"
    x = ref.bf16_value(E) if bf16 else ref.planes_value(E, e_scale)
    qe_ref, se_ref = ref.quantize_e(x)
    assert np.array_equal(np.concatenate(qe), qe_ref) and np.array_equal(np.concatenate(se).view(np.uint32), se_ref.view(np.uint32))
    assert se_ref[0, 5] == 0 and not qe_ref[0, 5].any()
    qq, sq = ref.quantize_q(qp, H)
    want = np.zeros((nq * B, d))
    for b in range(B):
        want[b::B] = ref.clip_out(qe_ref[b], se_ref[b], qq[b::B], sq[b::B], wv, bv)
    err = np.abs(out[:-1] - want).max()
    dist = np.abs(want - reference(lambda b: E[b], qp, wv, bv, B, H, nq)).max()
    print(f"err {err:.3e}, quantised to unquantised {dist:.3e}")
    assert dist > 100 * BAR, dist
    assert np.isfinite(out[:-1]).all() and err < BAR, err
    ne = n_nonempty(T, chunks)
    assert (ws[:-1, :, ne:, d] == M_EMPTY).all() and (ws[:-1, :, ne:, d + 1] == 0).all() and (ws[:-1, :, :ne, d + 1] > 0).all()


@pytest.mark.parametrize("kw", [dict(split=2, n_srcs=2), dict(only=(0, 3)), dict(omit=1), dict(omit=2), dict(omit=2, split=3, n_srcs=2)],
                         ids=["third-source-missing", "18-query-columns", "no-image", "no-scales", "no-scales-of-the-last-source"])
def test_launcher_refusals(eng, pkg, kw):
    """What launch_cross_absorbed refuses, and a missing image or scale array, is WT_ERR_INVALID_ARG before the launch."""
    B, H, T = 5, 6, 40
    E, qp, wv, bv = draw(np.random.default_rng(1), B, H, T, 3, False)
    kw = dict(kw)
    split = kw.pop("split", None)
    srcs = groups(E, split)[:kw.pop("n_srcs")] if split else [E]
    with pytest.raises(pkg.WtError) as err:
        eng.dbg_cross_absorbed_i8_chain(qp, srcs, wv, bv, B, H, T, 2, 3, split=split, **kw)
    assert err.value.code == 1
