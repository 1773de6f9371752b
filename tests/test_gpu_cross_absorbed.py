"""GPU (-m gpu): the absorbed cross-attention (k_cross_absorbed.hip) at the shapes the decoder chains run it, through
the chain-form tap wt_dbg_cross_absorbed_chain: several encoder batches per chain (split, e2..e4), empty key chunks,
rows up to the chain's width of 128, beam search's position loop (p0 > 0, ragged nq), the deferred maximum and the
other softmax edges, cross_absorbed_combine on hand-made records, the workspace discipline, and the whole absorbed
chain (host fold -> LN-fused query GEMM -> attention -> combine) against textbook cross-attention on the same weights.
References are float64 numpy, computed clip by clip ("What the absorbed chain's tests pin").

Budgets on inputs with the statistics of test_gpu_kernels.py (standard-normal E, scores O(3) in log2 units), from
there: 2e-5 absolute for the fp16-plane form, 4e-3 for the bf16 form on bf16-rounded E and q'."""
import numpy as np
import pytest

from test_gpu_decoder_step import bf16_round, check_ln_gemm, ln64

pytestmark = pytest.mark.gpu

WS_FILL = np.float32(-7.0)    # Engine.dbg_cross_absorbed_chain's pre-fill of ws ...
OUT_FILL = np.float32(-9.0)   # ... and of out
M_EMPTY = np.float32(-1e30) * np.float32(0.69314718055994530942)  # the m of a chunk without keys
FORMS = pytest.mark.parametrize("bf16", [False, True], ids=["planes", "bf16"])


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("micro")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def budget(bf16):
    return 4e-3 if bf16 else 2e-5


def rnd(bf16):
    return bf16_round if bf16 else (lambda a: a)


def draw(rng, B, H, T, nq, bf16, scale=3.0):
    """standard-normal E [B][T][d], queries with scores O(scale) in log2 units, Wv ~ 1 / sqrt(d), bv ~ 1"""
    d = 64 * H
    E = rnd(bf16)(rng.standard_normal((B, T, d), dtype=np.float32))
    qp = rnd(bf16)((rng.standard_normal((nq * B, H * d)) * (scale / np.sqrt(d))).astype(np.float32))
    wv = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    bv = rng.standard_normal(d).astype(np.float32)
    return E, qp, wv, bv


def groups(E, split):
    return [E[i:i + split] for i in range(0, E.shape[0], split)]


def clip_ref(Eb, Q, wv, bv):
    """One clip in float64: Eb [T][d], Q [n][H][d] (log2 domain) -> (out [n][H * 64], c [n][H][d], w [n][H][T])."""
    E64 = np.asarray(Eb, np.float64)
    n, H, d = Q.shape
    S = np.einsum("nhd,td->nht", Q.astype(np.float64), E64)
    P = np.exp2(S - S.max(axis=2, keepdims=True))
    w = P / P.sum(axis=2, keepdims=True)
    c = w @ E64
    out = np.einsum("hjd,nhd->nhj", wv.astype(np.float64).reshape(H, 64, d), c) + bv.astype(np.float64).reshape(H, 64)
    return out.reshape(n, H * 64), c, w


def reference(E_of, qp, wv, bv, B, H, nq):
    """[nq * B][d] float64, row = p * B + b, clip b against E_of(b)"""
    d = 64 * H
    ref = np.zeros((nq * B, d))
    for b in range(B):
        ref[b::B] = clip_ref(E_of(b), qp[b::B].reshape(nq, H, d), wv, bv)[0]
    return ref


def check_guards(out, ws):
    assert (out[-1] == OUT_FILL).all(), "out's guard row was written"
    assert (ws[-1] == WS_FILL).all(), "ws's guard row was written"


def run(eng, qp, E, wv, bv, B, H, T, chunks, nq, split=None, bf16=False, **kw):
    srcs = groups(E, split) if split else [E]
    out, ws = eng.dbg_cross_absorbed_chain(qp, srcs, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16, **kw)
    check_guards(out, ws)
    return out, ws


def n_nonempty(T, chunks):
    tiles = (T + 31) // 32
    tpc = (tiles + chunks - 1) // chunks
    return (tiles + tpc - 1) // tpc


# ---------------------------------------------------------------------------------------------- source routing ---
@FORMS
@pytest.mark.parametrize("B,H,split,T,chunks,nq", [
    (7, 6, 3, 97, 3, 2),     # three groups, the last of one clip
    (8, 6, 2, 200, 4, 1),    # four full groups
    (7, 8, 2, 97, 3, 1),     # four groups, a shorter last one; d_model 512: the 2-stage ring in the fp16 form
    (6, 8, 3, 130, 2, 2),    # two groups
    (64, 6, 32, 64, 2, 2),   # 64 = 2 x 32, the pipelined pair
    (5, 2, 4, 70, 2, 3),     # d_model 128
])
def test_every_row_reads_its_source_and_clip(eng, B, H, split, T, chunks, nq, bf16):
    """Clip b reads source b // split at clip b % split.  Every source is its own device allocation holding distinct
    data (and NaN where the group has no clip), so a wrong group, a wrong in-group offset or a wrong plane stride on a
    non-first source gives a row that misses its float64 reference by O(1), or NaN."""
    rng = np.random.default_rng(B * 131 + H * 17 + split + T + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    out, ws = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16)
    ref = reference(lambda b: E[b], qp, wv, bv, B, H, nq)
    err = np.abs(out[:-1] - ref).max(axis=1)
    assert np.isfinite(out[:-1]).all()
    assert err.max() < budget(bf16), (int(err.argmax()), err.max())


@FORMS
@pytest.mark.parametrize("H", [6, 8])
def test_scattering_clips_over_sources_changes_no_bit(eng, H, bf16):
    """The same seven clips as ONE encoder batch and scattered over four sources of two (the last of one): every record
    of ws and every output row is bit-identical — routing only selects bytes."""
    B, T, chunks, nq = 7, 161, 3, 2
    rng = np.random.default_rng(77 + H + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    one, ws_one = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, bf16=bf16)
    four, ws_four = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, split=2, bf16=bf16)
    assert np.array_equal(ws_one, ws_four)
    assert np.array_equal(one, four)
    ref = reference(lambda b: E[b], qp, wv, bv, B, H, nq)
    assert np.abs(one[:-1] - ref).max() < budget(bf16)


# -------------------------------------------------------------------------------------- the same bits every call ---
# the three smallest (T, chunks) of the routing list above (97 in 3 chunks at both widths) and 32 clips x 4 positions
REPEAT_CASES = [(64, 6, 32, 64, 2, 2), (5, 2, 4, 70, 2, 3), (7, 6, 3, 97, 3, 2), (7, 8, 2, 97, 3, 1), (32, 6, 8, 333, 4, 4)]
HUGE = np.float32([3e34, -7e33, 1e30, 5e36, -2e34, 1e25])


@FORMS
@pytest.mark.parametrize("B,H,split,T,chunks,nq", REPEAT_CASES)
def test_same_bits_every_call(eng, B, H, split, T, chunks, nq, bf16):
    """Six calls, each behind a call of the same shape whose E, workspace and output held huge values, so that every
    allocation the launch reuses is polluted: every call inside the float64 budget, records and output bit-identical to
    the first call's.  The probability planes are converted in registers just in front of the MFMAs that read them; an
    MFMA that takes such a register before the conversion has landed is a timing defect and shows between calls, not
    against the reference of one call (tools/isa_hazards.py holds the distance in the ISA)."""
    rng = np.random.default_rng(B * 131 + H * 17 + split + T + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    ref = reference(lambda b: E[b], qp, wv, bv, B, H, nq)
    first = None
    for rep in range(6):
        eng.dbg_cross_absorbed_chain(qp, groups(E * HUGE[rep], split), wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16,
                                     ws_fill=HUGE[rep], out_fill=HUGE[rep])
        out, ws = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16)
        err = np.abs(out[:-1] - ref).max()
        assert np.isfinite(out[:-1]).all() and err < budget(bf16), (rep, err)
        first = (out, ws) if first is None else first
        assert np.array_equal(ws, first[1]) and np.array_equal(out, first[0]), f"call {rep} differs from call 0"


# ------------------------------------------------------------------------------------------------ empty chunks ---
@FORMS
@pytest.mark.parametrize("T,chunks", [(1500, 13), (1500, 15), (97, 3), (64, 16), (33, 2), (32, 1), (1, 1), (1, 4)])
def test_empty_key_chunks(eng, T, chunks, bf16):
    """tiles_per_chunk = ceil(tiles / chunks) leaves the last chunks without keys (T = 1500: 47 tiles in 13 or 15 chunks
    of 4 tiles, 12 of them non-empty).  Such a chunk records c = 0, l = 0 and m = -1e30 ln 2, which the combine weights
    with exp(m - max m) = 0 exactly.  The launcher accepts chunks > tiles (T = 64 in 16 chunks, T = 1 in 4): the engine
    never asks for it (n_abs is clamped to the tile count) but the records make it correct, so it is pinned here rather
    than refused.  The output equals float64, and equals the call with only the non-empty chunks: their key ranges are
    the same, so their records are bit-identical."""
    B, H, nq = 2, 6, 2
    d, rows = 64 * H, nq * B
    rng = np.random.default_rng(T * 31 + chunks + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    out, ws = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, bf16=bf16)
    full = n_nonempty(T, chunks)
    assert {(1500, 13): 12, (1500, 15): 12, (97, 3): 2, (64, 16): 2, (33, 2): 2, (32, 1): 1, (1, 1): 1, (1, 4): 1}[(T, chunks)] == full
    rec = ws[:rows]
    assert (rec[:, :, :full, d + 1] > 0).all()                     # l of a chunk with keys
    assert (rec[:, :, full:, :d] == 0).all() and (rec[:, :, full:, d + 1] == 0).all()
    assert (rec[:, :, full:, d] < -6e29).all()                     # -1e30 ln 2
    m_max = rec[:, :, :, d].max(axis=2, keepdims=True)
    assert (np.exp(rec[:, :, full:, d] - m_max) == 0).all()        # the combine's weight, in its own fp32
    ref = reference(lambda b: E[b], qp, wv, bv, B, H, nq)
    assert np.abs(out[:-1] - ref).max() < budget(bf16)
    if full < chunks:
        assert n_nonempty(T, full) == full
        out2, ws2 = run(eng, qp, E, wv, bv, B, H, T, full, nq, bf16=bf16)
        assert np.abs(out2[:-1] - out[:-1]).max() < budget(bf16)
        tiles = (T + 31) // 32
        assert -(-tiles // full) == -(-tiles // chunks)            # the same tiles_per_chunk: the same key ranges
        assert np.array_equal(ws2[:rows], rec[:, :, :full])


# ------------------------------------------------------------------------------------------------- chain width ---
@pytest.mark.parametrize("B,H,split,T,chunks,nq,bf16", [
    (64, 6, 32, 333, 2, 2, False), (64, 6, 32, 333, 2, 2, True),    # 64 clips x 2 prompt positions, two sources
    (32, 6, 8, 333, 4, 4, False), (32, 6, 8, 333, 4, 4, True),      # 32 x 4, four sources, two launches (p0 = 0, 2)
    (32, 8, 8, 333, 4, 4, False), (32, 8, 8, 333, 4, 4, True),      # 8 heads: two positions per launch
    (64, 8, 32, 1500, 2, 2, False), (64, 6, 32, 1500, 2, 2, True),  # the full sweep at a pair's width
])
def test_rows_at_the_chains_width(eng, B, H, split, T, chunks, nq, bf16):
    """128 rows: row = (p0 + qpos) * B + b into qp and ws at the decoder's widest, every row against float64."""
    assert nq * B == 128
    rng = np.random.default_rng(B + H + T + nq + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    out, ws = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16)
    ref = reference(lambda b: E[b], qp, wv, bv, B, H, nq)
    err = np.abs(out[:-1] - ref).max(axis=1)
    assert err.max() < budget(bf16), (int(err.argmax()), err.max())


# ------------------------------------------------------------------------------------------ beam position loop ---
@FORMS
@pytest.mark.parametrize("clips,H,K", [(3, 6, 5), (2, 6, 8), (3, 8, 5), (16, 6, 8)])
def test_beam_hypotheses_as_query_positions(eng, clips, H, K, bf16):
    """decode_beam rides the K hypotheses of a clip as query positions: 6 heads take p0 = 0, 2, 4, 6 (K = 5: the last
    launch has nq = 1), 8 heads p0 = 0, 2, 4.  chunks as decode_beam picks them: min(16, ceil(256 / clips), tiles)."""
    T = 1500
    chunks = min(16, -(-256 // clips), (T + 31) // 32)
    rng = np.random.default_rng(clips * 100 + H + K + int(bf16))
    E, qp, wv, bv = draw(rng, clips, H, T, K, bf16)
    out, ws = run(eng, qp, E, wv, bv, clips, H, T, chunks, K, bf16=bf16)
    ref = reference(lambda b: E[b], qp, wv, bv, clips, H, K)
    err = np.abs(out[:-1] - ref).max(axis=1)
    assert err.max() < budget(bf16), (int(err.argmax()), err.max())


# ------------------------------------------------------------------------------ row independence, ws discipline ---
@FORMS
def test_rows_depend_on_their_own_clip_and_query_only(eng, bf16):
    """Another clip's E, or another row's q', changes no bit of a row's records or output."""
    B, H, T, chunks, nq, split = 5, 6, 130, 3, 3, 2
    rng = np.random.default_rng(5 + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    base, ws0 = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16)
    E2 = E.copy()
    E2[3] = rnd(bf16)(rng.standard_normal(E[3].shape, dtype=np.float32))   # same magnitude: the shared e_scale stays
    out, ws = run(eng, qp, E2, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16)
    same = np.arange(nq * B) % B != 3
    assert np.array_equal(out[:-1][same], base[:-1][same]) and np.array_equal(ws[:-1][same], ws0[:-1][same])
    assert (np.abs(out[:-1][~same] - base[:-1][~same]).max(axis=1) > 1e-2).all()
    qp2 = qp.copy()
    r = 2 * B + 1
    qp2[r] = rnd(bf16)((rng.standard_normal(qp[r].shape) * (3.0 / np.sqrt(64 * H))).astype(np.float32))
    out, ws = run(eng, qp2, E, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16)
    same = np.arange(nq * B) != r
    assert np.array_equal(out[:-1][same], base[:-1][same]) and np.array_equal(ws[:-1][same], ws0[:-1][same])
    assert np.abs(out[r] - base[r]).max() > 1e-2


@FORMS
@pytest.mark.parametrize("H,nq,only", [(6, 5, (2, 2)), (6, 5, (4, 1)), (8, 5, (2, 2)), (2, 9, (8, 1)), (6, 3, (0, 2))])
def test_one_launch_writes_its_positions_records_only(eng, H, nq, only, bf16):
    """A launch over positions p0 .. p0 + nq - 1 writes exactly the records of rows (p0 + qpos) * B + b: the records
    of every other position keep the pre-fill, c, m, l and the pad; the launched rows equal the whole chain's, bit for
    bit; guard rows stay."""
    B, T, chunks, split = 3, 100, 2, 2
    d = 64 * H
    rng = np.random.default_rng(H * 10 + nq + only[0] + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    whole, ws_whole = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16)
    out, ws = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16, only=only)
    p = np.arange(nq * B) // B
    hit = (p >= only[0]) & (p < only[0] + only[1])
    assert (ws[:-1][~hit] == WS_FILL).all()
    assert (ws[:-1][hit][..., d + 2:] == WS_FILL).all()            # the pad of a written record
    assert np.array_equal(ws[:-1][hit][..., :d + 2], ws_whole[:-1][hit][..., :d + 2])
    assert np.array_equal(out[:-1][hit], whole[:-1][hit])
    ref = reference(lambda b: E[b], qp, wv, bv, B, H, nq)
    assert np.abs(out[:-1][hit] - ref[hit]).max() < budget(bf16)


def test_refused_shapes_return_invalid_arg(eng, pkg):
    """What the launcher (or the tap, for its own buffers) refuses comes back as WT_ERR_INVALID_ARG before a launch."""
    B, H, T = 5, 6, 40
    rng = np.random.default_rng(1)
    E, qp, wv, bv = draw(rng, B, H, T, 3, False)

    def refused(**kw):
        a = dict(batch=B, heads=H, T=T, chunks=2, nq=3, split=None, srcs=[E])
        a.update(kw)
        with pytest.raises(pkg.WtError) as ei:
            eng.dbg_cross_absorbed_chain(qp, a["srcs"], wv, bv, a["batch"], a["heads"], a["T"], a["chunks"], a["nq"],
                                         split=a["split"], only=a.get("only"))
        assert ei.value.code == 1

    refused(split=1, srcs=groups(E, 1)[:4])                 # five groups of one clip
    refused(split=2, srcs=groups(E, 2)[:2])                 # three groups, the third source missing
    refused(only=(0, 3))                                    # 3 positions x 6 heads > 16 query columns in one launch
    refused(only=(2, 2))                                    # past the nq positions of qp and ws
    refused(chunks=17)
    refused(split=3)                                        # one source must hold the whole batch
    refused(T=0)
    out, ws = eng.dbg_cross_absorbed_chain(qp, [E], wv, bv, B, H, T, 2, 3)   # and the engine still works
    assert np.abs(out[:-1] - reference(lambda b: E[b], qp, wv, bv, B, H, 3)).max() < 2e-5


# ------------------------------------------------------------------------------------------------ softmax edges ---
def edge_bound(E, qp, wv, bv, B, H, nq, bf16, T_chunk):
    """Per-element bound [nq * B][d] on |kernel - float64| from the float64 reference and the roundings alone.
    Scores (log2 units): fp16 planes carry 22 bits of q' and of E (2 * 2^-22 per product) and fp32 accumulation of
    d products is taken as sqrt(d) 2^-24, both relative to A_j = sum_i |q'_i e_ji|; the bf16 form has exact products of
    its rounded operands and the same accumulation:  ds = max_j A_j (2^-21 + sqrt(d) 2^-24).
    Probabilities: p_j = exp2(s_j - m) 2^12 is off by ds ln 2 relative, plus 2^-20 for v_exp_f32, the two-plane split
    (2^-22) and the alpha rescales; the bf16 form rounds p to bf16, 2^-8 relative at worst:  eps_p.
    Context c = sum_j w_j e_j, w = p / sum p: to first order dc = sum_j w_j eta_j (e_j - c) with |eta_j| <= eps_p, plus
    the planes of E (2^-21 |e|, fp16 form) and fp32 accumulation over the chunk's keys (sqrt(T_chunk) 2^-24):
      dc <= eps_p sum_j w_j |e_j - c| + (2^-21 + sqrt(T_chunk) 2^-24) sum_j w_j |e_j|.
    Output: |Wv_h| dc plus the combine's fp32 (2^-21 (|Wv_h| |c| + |bv|): __expf weights, 1 / l, d products).
    The allowed margin over this model is a factor 2."""
    d = 64 * H
    bound = np.zeros((nq * B, d))
    aW = np.abs(wv.astype(np.float64)).reshape(H, 64, d)
    for b in range(B):
        E64 = E[b].astype(np.float64)
        Q = qp[b::B].reshape(nq, H, d).astype(np.float64)
        _, c, w = clip_ref(E[b], qp[b::B].reshape(nq, H, d), wv, bv)
        A = np.einsum("nhd,td->nht", np.abs(Q), np.abs(E64)).max(axis=2)              # [nq][H]
        ds = A * (2.0 ** -21 + np.sqrt(d) * 2.0 ** -24)
        eps_p = ds * np.log(2.0) + 2.0 ** -20 + (2.0 ** -8 if bf16 else 0.0)
        spread = np.einsum("nht,nhtd->nhd", w, np.abs(E64[None, None] - c[:, :, None, :]))
        mass = w @ np.abs(E64)
        dc = eps_p[:, :, None] * spread + (2.0 ** -21 + np.sqrt(T_chunk) * 2.0 ** -24) * mass
        do = np.einsum("hjd,nhd->nhj", aW, dc) + 2.0 ** -21 * (
            np.einsum("hjd,nhd->nhj", aW, np.abs(c)) + np.abs(bv.astype(np.float64)).reshape(H, 64))
        bound[b::B] = 2.0 * do.reshape(nq, d)
    return bound


def check_edge(eng, E, qp, wv, bv, B, H, T, chunks, nq, bf16):
    out, ws = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, bf16=bf16)
    ref = reference(lambda b: E[b], qp, wv, bv, B, H, nq)
    tpc = -(-((T + 31) // 32) // chunks) * 32
    bound = edge_bound(E, qp, wv, bv, B, H, nq, bf16, min(T, tpc))
    err = np.abs(out[:-1] - ref)
    assert np.isfinite(out[:-1]).all()
    assert (err <= bound).all(), (err.max(), (err / bound).max())
    return out, ws, ref


def planted(rng, B, H, T, nq, bf16, keys, scores, base=0.3):
    """E = base * noise with rows `keys` of every clip replaced by (score / |u|^2) u + noise, every head's q' = u + small
    noise: key k scores ~ scores[k] log2 units above a background of O(base)."""
    d = 64 * H
    u = rng.standard_normal(d) / np.sqrt(d)
    E = base * rng.standard_normal((B, T, d))
    for k, s in zip(keys, scores):
        E[:, k] += s / (u @ u) * u
    qp = u[None, None, :] + 0.1 * rng.standard_normal((nq * B, H, d)) / np.sqrt(d)
    E, qp = rnd(bf16)(E.astype(np.float32)), rnd(bf16)(qp.reshape(nq * B, H * d).astype(np.float32))
    wv = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    bv = rng.standard_normal(d).astype(np.float32)
    return E, qp, wv, bv


@FORMS
@pytest.mark.parametrize("H", [6, 8])
@pytest.mark.parametrize("order", ["rising", "falling"])
def test_maximum_grows_across_the_deferral_threshold(eng, H, order, bf16):
    """The running maximum is raised only when a tile's maximum exceeds it by more than kDeferA = 3 log2 units.  One
    planted key per tile makes the tile maxima grow by 0.5, 2.9, 3.1 and 9.0 (deferred, deferred — the probabilities
    then reach 2^12 2^2.9 —, raised, raised), or fall by the same steps; one chunk, so that one block sees every step,
    and two.  Bound: edge_bound."""
    B, nq, T = 2, 2, 5 * 32 + 7
    levels = np.cumsum([10.0, 0.5, 2.9, 3.1, 9.0])
    if order == "falling":
        levels = levels[::-1]
    rng = np.random.default_rng(H + len(order) + int(bf16))
    E, qp, wv, bv = planted(rng, B, H, T, nq, bf16, [32 * t + 5 + t for t in range(5)], levels)
    for chunks in (1, 2):
        check_edge(eng, E, qp, wv, bv, B, H, T, chunks, nq, bf16)


@FORMS
@pytest.mark.parametrize("where", ["first_tile", "last_partial_tile", "second_chunk"])
def test_one_dominating_key(eng, where, bf16):
    """One key 40 log2 units above the rest takes the whole weight, wherever it sits: the first tile, the ragged last
    tile of the clip (T = 107: keys 96 .. 106), a chunk other than the first (whose records then combine with weights
    2^-40).  The output is Wv e_key + bv; bound: edge_bound."""
    B, H, nq, T, chunks = 2, 6, 2, 107, 2
    key = {"first_tile": 3, "last_partial_tile": 105, "second_chunk": 70}[where]
    rng = np.random.default_rng(key + int(bf16))
    E, qp, wv, bv = planted(rng, B, H, T, nq, bf16, [key], [40.0])
    out, ws, ref = check_edge(eng, E, qp, wv, bv, B, H, T, chunks, nq, bf16)
    one_hot = reference(lambda b: E[b, key:key + 1], qp, wv, bv, B, H, nq)
    assert np.abs(ref - one_hot).max() < 1e-6      # the case is what it says


@FORMS
@pytest.mark.parametrize("H,T,chunks", [(6, 97, 2), (8, 1500, 15), (2, 33, 1)])
def test_equal_scores_give_the_mean(eng, H, T, chunks, bf16):
    """q' = 0: every key weighs 1 / T and the result is Wv mean(E) + bv, empty chunks and ragged tiles included (the
    column maximum 0 takes the unscaled branch of the query split).  Bound: edge_bound (ds = 0)."""
    B, nq = 2, 2
    rng = np.random.default_rng(H + T + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    qp[:] = 0
    out, ws, ref = check_edge(eng, E, qp, wv, bv, B, H, T, chunks, nq, bf16)
    mean = np.stack([wv.astype(np.float64) @ E[r % B].astype(np.float64).mean(0) + bv for r in range(nq * B)])
    assert np.abs(ref - mean).max() < 1e-12


@FORMS
def test_tiny_queries_keep_the_mask(eng, bf16):
    """The lower edge of the admissible |q'| (DESIGN): max |q'| = 2^-80.  All scores vanish, the result is the mean over
    the T real keys; keys past T in the ragged last tile (they re-read row T - 1) must stay masked although the fp16
    form multiplies raw scores, the mask included, by s_inv ~ 2^-94 / e_scale.  A finite mask of -1e30 gave them weight
    1 there: row T - 1 counted 32 - T % 32 extra times, an O(0.1) error.  Bound: edge_bound."""
    B, H, nq, T, chunks = 2, 6, 2, 33, 1
    rng = np.random.default_rng(3 + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    qp = rnd(bf16)((qp * np.float32(2.0 ** -80 / np.abs(qp).max())).astype(np.float32))
    check_edge(eng, E, qp, wv, bv, B, H, T, chunks, nq, bf16)
    check_edge(eng, E, qp, wv, bv, B, H, T, 2, nq, bf16)


@FORMS
def test_a_chunk_whose_weight_underflows(eng, bf16):
    """Chunk 1 holds a key 200 log2 units above everything in chunk 0: chunk 0's weight exp(m_0 - m_1) ~ 2^-200
    underflows to 0 in the combine, and the result is chunk 1's alone.  Bound: edge_bound."""
    B, H, nq, T, chunks = 2, 6, 2, 128, 2
    rng = np.random.default_rng(9 + int(bf16))
    E, qp, wv, bv = planted(rng, B, H, T, nq, bf16, [100], [200.0])
    out, ws, ref = check_edge(eng, E, qp, wv, bv, B, H, T, chunks, nq, bf16)
    d = 64 * H
    m = ws[:nq * B, :, :, d]
    assert (np.exp(m[:, :, 0] - m[:, :, 1]) == 0).all()


@FORMS
def test_all_zero_clip_gives_bv_exactly(eng, bf16):
    """E = 0 for one clip: its planes are zeros, every context sum is 0 (of either sign), c / l = 0 and the output is
    0 + bv = bv EXACTLY, not within an ulp.  The other clips keep the shared e_scale away from its default."""
    B, H, nq, T, chunks = 3, 6, 2, 97, 2
    rng = np.random.default_rng(21 + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    E[1] = 0
    out, ws = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, split=2, bf16=bf16)
    for p in range(nq):
        assert np.array_equal(out[p * B + 1], bv)
    ref = reference(lambda b: E[b], qp, wv, bv, B, H, nq)
    assert np.abs(out[:-1] - ref).max() < budget(bf16)


@FORMS
@pytest.mark.parametrize("H", [6, 8])
def test_largest_admissible_queries(eng, H, bf16):
    """The upper edge of the admissible range (DESIGN): max_j sum_i |q'_i e_ji| = 2^12, a hundred times the decoder's.
    The query split scales each column's largest element into [2^14, 2^15) whatever its size, so nothing overflows; what
    grows is the fp32 rounding of the scores themselves, ds = 2^12 (2^-21 + sqrt(d) 2^-24) ~ 8e-3 log2 units, and with
    it edge_bound.  Scores spread over hundreds of log2 units: a few keys carry the weight."""
    B, nq, T, chunks = 2, 2, 200, 3
    d = 64 * H
    rng = np.random.default_rng(40 + H + int(bf16))
    E, qp, wv, bv = draw(rng, B, H, T, nq, bf16)
    A = max(np.einsum("rhd,td->rht", np.abs(qp[b::B].reshape(nq, H, d)).astype(np.float64),
                      np.abs(E[b]).astype(np.float64)).max() for b in range(B))
    qp = rnd(bf16)((qp * np.float32(4096.0 / A)).astype(np.float32))
    check_edge(eng, E, qp, wv, bv, B, H, T, chunks, nq, bf16)


# ------------------------------------------------------------------------------------------------ combine alone ---
@pytest.mark.parametrize("H", [2, 6, 8])
def test_combine_on_hand_made_records(eng, H):
    """cross_absorbed_combine alone: c = sum_k w_k c_k / sum_k w_k l_k, w_k = exp(m_k - max m), then Wv_h c + bv_h with
    Wv in cross_q_layout order; d_model 128, 384, 512.  Rows: random m within +-4; chunks without keys (c = 0, l = 0,
    m = -1e30 ln 2) among real ones; a single surviving chunk; the same m in every chunk.
    Bound: __expf of |x| <= 8 is 2^-20 relative, the fp32 sums over 5 chunks and d products and 1 / l add a few 2^-24:
    2^-19 (|Wv_h| |c| + |bv|) per element, a factor 2 over that model."""
    d, rows, chunks = 64 * H, 6, 5
    rng = np.random.default_rng(H)
    ws = np.full((rows + 1, H, chunks, d + 4), WS_FILL, np.float32)
    ws[:rows, :, :, :d] = rng.standard_normal((rows, H, chunks, d))
    ws[:rows, :, :, d] = rng.uniform(-4, 4, (rows, H, chunks))
    ws[:rows, :, :, d + 1] = rng.uniform(0.5, 30, (rows, H, chunks))
    empty = np.zeros((rows, chunks), bool)
    empty[1, [3, 4]] = True              # trailing empty chunks, as the attention leaves them
    empty[2, [0, 2]] = True              # ... and anywhere else
    empty[3, [0, 1, 2, 4]] = True        # one survivor
    ws[4, :, :, d] = 1.25                # equal m
    ws[5, :, :, d] = np.float32(-60.0) * np.arange(chunks)   # all but chunk 0 negligible, the last two underflow
    for r, k in zip(*np.nonzero(empty)):
        ws[r, :, k, :d], ws[r, :, k, d], ws[r, :, k, d + 1] = 0, M_EMPTY, 0
    wv = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    bv = rng.standard_normal(d).astype(np.float32)
    out, ws_back = eng.dbg_cross_absorbed_chain(None, None, wv, bv, rows, H, 1, chunks, 1, combine_only=True, ws=ws)
    assert np.array_equal(ws_back, ws)                       # the combine reads ws only
    assert (out[-1] == OUT_FILL).all()
    W = ws[:rows].astype(np.float64)
    m = W[..., d]
    w = np.exp(m - m.max(axis=2, keepdims=True))
    c = np.einsum("rhk,rhkd->rhd", w, W[..., :d]) / (w * W[..., d + 1]).sum(axis=2)[..., None]
    W64 = wv.astype(np.float64).reshape(H, 64, d)
    ref = (np.einsum("hjd,rhd->rhj", W64, c) + bv.astype(np.float64).reshape(H, 64)).reshape(rows, d)
    bound = 2.0 ** -19 * (np.einsum("hjd,rhd->rhj", np.abs(W64), np.abs(c)) + np.abs(bv).reshape(H, 64)).reshape(rows, d)
    err = np.abs(out[:rows] - ref)
    assert (err <= bound).all(), (err.max(), (err / bound).max())


# ----------------------------------------------------------------------- the chain against real cross-attention ---
@FORMS
@pytest.mark.parametrize("H", [6, 8])
def test_absorbed_chain_is_cross_attention(eng, pkg, H, bf16):
    """softmax((Wq LN(x) + bq) . (Wk e) / 8) (Wv e + bv) through the absorbed chain on the same weights: the host fold
    (A, a), the LN-fused query GEMM with W = A, bias = a, the attention over E from two sources, the combine.
    Stage 1: q' against float64 LN(x) A^T + a at the LN-GEMM's budget (check_ln_gemm: 5e-6 of the largest element, plus
      the bf16 form's rounding slack).
    Stage 2: the attention against float64 on the q' it was given (bf16-rounded in the bf16 form, as the kernel rounds
      it) and E: 2e-5 / 4e-3.
    End to end against the float64 textbook form (on bf16-rounded E in the bf16 form): the stage-2 budget plus q''s error
      through the softmax.  With |dq'_i| <= bar (stage 1's bar, 5e-6 of the largest q') every score moves by at most
      Ds = max_j sum_i bar |e_ji|, every weight by a factor within 2^(+-2 Ds), so
      |dc| <= (2^(2 Ds) - 1) sum_j w_j |e_j - c| and |do| <= |Wv_h| |dc|: computed below from the reference alone.
      The bf16 form also rounds LN(x), A and then q' to bf16, 2^-8 relative at worst per factor; a worst-case sum of
      those over d x d products says nothing, so they enter as independent errors: sigma_i = 2^-8 sqrt(sum_k (LN_k
      A_ik)^2 + q'_i^2) per element of q' (each product's bound taken as its deviation), a score's deviation
      sqrt(sum_i (sigma_i e_ji)^2), and Ds grows by 6 of those (8 rows x heads x 200 keys = 1e4 scores).
    The cached form (dbg_cross_attention, fp32 cache) on kc = Wk E, vc = Wv E + bv sits within its own 2e-5 of the same
    textbook reference (plus 1e-6 for the cache's rounding to fp32)."""
    B, nq, T, chunks, split = 4, 2, 200, 3, 2
    d, rows = 64 * H, nq * B
    rng = np.random.default_rng(H * 3 + int(bf16))
    x = (rng.standard_normal((rows, d)) * 2 + 0.3).astype(np.float32)
    g_, b_ = (1 + 0.2 * rng.standard_normal(d)).astype(np.float32), (0.1 * rng.standard_normal(d)).astype(np.float32)
    wq, wk, wv = ((rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32) for _ in range(3))
    bq, bv = (0.1 * rng.standard_normal(d)).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    E = rnd(bf16)(rng.standard_normal((B, T, d), dtype=np.float32))
    A, a = pkg.absorbed_query_matrix(wq, bq, wk)

    ln = ln64(x, g_, b_)
    qp, _ = eng.dbg_dec_ln_gemm(A, a, g_, b_, xin=x, bf16=bf16)
    check_ln_gemm(qp, ln, b_, A, a, False, bf16)                                            # stage 1
    out, ws = run(eng, qp, E, wv, bv, B, H, T, chunks, nq, split=split, bf16=bf16)
    given = rnd(bf16)(qp)
    ref2 = reference(lambda b: E[b], given, wv, bv, B, H, nq)
    assert np.abs(out[:-1] - ref2).max() < budget(bf16)                                     # stage 2

    q64 = ln @ wq.astype(np.float64).T + bq
    Wk64, Wv64 = wk.astype(np.float64), wv.astype(np.float64)
    qp64 = ln @ A.astype(np.float64).T + a
    bar = np.full(qp64.shape, 5e-6 * np.abs(qp64).max())
    if bf16:
        A2 = A.astype(np.float64) ** 2
        sig = 2.0 ** -8 * np.sqrt((ln ** 2) @ A2.T + qp64 ** 2)
    text = np.zeros((rows, d))
    bound = np.zeros((rows, d))
    kc = np.zeros((B, H, T, 64), np.float32)
    vc = np.zeros((B, H, T, 64), np.float32)
    for b in range(B):
        E64 = E[b].astype(np.float64)
        k, v = E64 @ Wk64.T, E64 @ Wv64.T + bv
        kc[b], vc[b] = k.reshape(T, H, 64).transpose(1, 0, 2), v.reshape(T, H, 64).transpose(1, 0, 2)
        for p in range(nq):
            r = p * B + b
            for h in range(H):
                sl = slice(64 * h, 64 * h + 64)
                s = k[:, sl] @ q64[r, sl] / 8.0
                w = np.exp(s - s.max())
                w /= w.sum()
                text[r, sl] = w @ v[:, sl]
                c = w @ E64
                Ds = (np.abs(E64) @ bar[r, h * d:(h + 1) * d]).max()
                if bf16:
                    Ds += 6.0 * np.sqrt((E64 ** 2) @ (sig[r, h * d:(h + 1) * d] ** 2)).max()
                dc = (np.exp2(2.0 * Ds) - 1.0) * (w @ np.abs(E64 - c))
                bound[r, sl] = budget(bf16) + np.abs(Wv64[sl]) @ dc
    # the absorbed scores are the textbook's: the two float64 forms agree
    assert np.abs(reference(lambda b: E[b], qp64.astype(np.float32), wv, bv, B, H, nq) - text).max() < 1e-4
    err = np.abs(out[:-1] - text)
    assert (err <= bound).all(), (err.max(), (err / bound).max())                           # end to end
    cached = eng.dbg_cross_attention(x, g_, b_, wq, bq, kc, vc, chunks=2, nq=nq)
    assert np.abs(cached - text).max() < 2e-5 + 1e-6
