"""GPU (-m gpu): the log-mel front end kernel by kernel, off the 30 s geometry, through the debug taps of
include/wt_debug.h (wt_dbg_pcm_to_planes, wt_dbg_log_clipmax, wt_dbg_mel_normalize, wt_dbg_mel_transpose,
wt_dbg_frontend_stages).  Every reference is float64 numpy computed from that kernel's OWN inputs, so a stage is judged
alone and a whole-path failure can be pinned on one of the seven launches of Engine::logmel.

The split bound used for every pair of fp16 planes (pcm_to_planes, mel_transpose_planes<false>), derived from
split_f16x2 / split_f16 in csrc/bf16_split.h: with a = x * scale (scale a power of two: exact), hi = fp16(a) rounded to
nearest even and lo = fp16(a - hi).  For 2^e <= |a| < 2^(e+1) inside fp16's normal range |a - hi| <= 2^(e-11) (half an
ulp of an 11-bit significand), and a - hi is exact in fp32 (hi holds the top 11 of a's 24 bits).  Rounding that
remainder to fp16 costs at most 2^-11 of it while it is a normal fp16, i.e. 2^(e-22) <= 2^-22 |a|, and at most half a
subnormal step, 2^-25, once it (or a itself) falls below 2^-14.  Hence
    |hi + lo - a| <= max(2^-22 |a|, 2^-25)        for |a| <= 65504."""
import numpy as np
import pytest

from conftest import synth_pcm

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-4      # |delta| on the normalised log-mel: the whole-path bar of test_gpu_path.py
PCM_BOUND = 32.0    # Engine::kPcmBound
PCM_SCALE = 512.0   # f16_scale_for(32): 32 * 512 = 2^14, a factor 4 under fp16's largest value
NEG_INF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def eng(pkg, assets):
    # "tiny" is the smallest synthetic model with the reference's 30 s window (3000 frames); every model's vocab file
    # carries the 80 x 201 bank
    prefix, vocab = assets("tiny")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def split_bound(a):
    a = np.abs(np.asarray(a, np.float64))
    return np.maximum(a * 2.0 ** -22, 2.0 ** -25)


def check_split(hi, lo, a, what):
    """hi / lo float16 arrays against a = float32(x * scale)."""
    a = np.asarray(a, np.float32)
    assert np.array_equal(hi.view(np.uint16), a.astype(np.float16).view(np.uint16)), what + ": hi != fp16(x * scale)"
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - a.astype(np.float64))
    worst = (err / split_bound(a)).max()
    print(f"{what}: |hi + lo - a| at most {worst:.3f} of the split bound")
    assert (err <= split_bound(a)).all(), what


# ------------------------------------------------------------------------------------------------ pcm_to_planes ---

@pytest.mark.parametrize("n", [8, 36, 1028])
def test_pcm_to_planes(eng, n):
    """Four clips of n samples at an out_stride larger than the clip, 8 guard elements behind the last clip.  Clip 0
    sits on a 2^-10 grid (exact in two fp16 planes at scale 512: 16 significant bits), clip 1 is random (hi and the split
    bound of the module docstring), clip 2 starts with +-31.999, +-32, +-32.001, +-1e30 and clip 3 holds +-inf: values at
    and beyond +-limit clamp to +-limit exactly, 31.999 passes.  A NaN in clip 3 stays a NaN in place, its three
    neighbours in the same 4-vector are converted as usual.  Everything the kernel does not own (the gaps between
    clips, the guard) comes back bit for bit."""
    rng = np.random.default_rng(n)
    B, stride, guard = 4, (n + 7) // 8 * 8 + 8, 8
    pcm = rng.uniform(-1, 1, (B, n)).astype(np.float32)
    pcm[0] = rng.integers(-32768, 32769, n).astype(np.float32) * np.float32(2.0 ** -10)
    pcm[1] = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32).clip(-31, 31)
    pcm[2, :8] = [31.999, -31.999, 32.0, -32.0, 32.001, -32.001, 1e30, -1e30]
    pcm[3, 1] = np.nan  # 4-vector 0 of clip 3: elements 0, 2, 3 are its neighbours
    pcm[3, 4:6] = [np.inf, -np.inf]
    fill = rng.integers(0, 0x7000, (2, B * stride + guard)).astype(np.uint16).view(np.float16)
    out = eng.dbg_pcm_to_planes(pcm, fill, stride, PCM_SCALE, PCM_BOUND)
    hi, lo = out[0, :B * stride].reshape(B, stride), out[1, :B * stride].reshape(B, stride)
    # not the kernel's to write
    assert np.array_equal(out[:, B * stride:].view(np.uint16), fill[:, B * stride:].view(np.uint16)), "guard written"
    assert np.array_equal(out[:, :B * stride].reshape(2, B, stride)[:, :, n:].view(np.uint16),
                          fill[:, :B * stride].reshape(2, B, stride)[:, :, n:].view(np.uint16)), "gap between clips written"
    # the grid clip is exact
    back = (hi[0, :n].astype(np.float64) + lo[0, :n].astype(np.float64)) / PCM_SCALE
    assert np.array_equal(back, pcm[0].astype(np.float64))
    # everything that is not the NaN: hi and the split bound against the CLAMPED sample
    want = np.clip(pcm, -PCM_BOUND, PCM_BOUND) * np.float32(PCM_SCALE)
    ok = ~np.isnan(pcm)
    for b in range(B):
        check_split(hi[b, :n][ok[b]], lo[b, :n][ok[b]], want[b][ok[b]], f"pcm_to_planes n={n} clip {b}")
    # the clamp, stated
    top = PCM_BOUND * PCM_SCALE
    assert np.array_equal(hi[2, 2:8].astype(np.float64), [top, -top] * 3) and (lo[2, 2:8].astype(np.float64) == 0).all()
    assert np.array_equal(hi[3, 4:6].astype(np.float64), [top, -top]) and (lo[3, 4:6].astype(np.float64) == 0).all()
    below = hi[2, :2].astype(np.float64) + lo[2, :2].astype(np.float64)
    assert (np.abs(below) < top).all() and np.abs(below / PCM_SCALE - [31.999, -31.999]).max() < 4e-6
    # the NaN
    assert np.isnan(hi[3, 1]) and np.isnan(lo[3, 1])
    assert not np.isnan(hi[3, :n][ok[3]]).any() and not np.isnan(lo[3, :n][ok[3]]).any()


def test_pcm_to_planes_refuses_bad_shapes(eng, pkg):
    fill = np.zeros((2, 24), np.float16)
    for pcm, stride in [(np.zeros((1, 6), np.float32), 16),    # n % 4
                        (np.zeros((1, 8), np.float32), 12),    # out_stride % 8
                        (np.zeros((1, 16), np.float32), 8)]:   # out_stride < n
        with pytest.raises(pkg.WtError) as ei:
            eng.dbg_pcm_to_planes(pcm, fill, stride, PCM_SCALE, PCM_BOUND)
        assert ei.value.code == 1
    with pytest.raises(pkg.WtError):
        eng.dbg_pcm_to_planes(np.zeros((1, 8), np.float32), np.zeros((2, 18), np.float16), 16, PCM_SCALE, PCM_BOUND)  # plane % 4


# -------------------------------------------------------------------------------------------------- log_clipmax ---

CLIPMAX_SHAPES = [(1, 32, 32, 128), (2, 70, 80, 128), (3, 33, 33, 128), (1, 129, 80, 128)]
EPS32 = np.float32(1e-10)


def clipmax_input(B, T, n_mel, ld, seed):
    """melacc [B][T][ld]: 1e-12 .. 1e3 scaled down by 1e3 per clip (clip 1's maximum is negative in log10, and a
    maximum taken from the wrong clip is off by ~3), exact zeros, negatives, the floor value itself and its float
    neighbours; columns >= n_mel hold 1e30 (a column read past n_mel would own every maximum); the single largest
    value of clip 0, 1e6, sits in the LAST frame, i.e. beyond every t_valid < T."""
    rng = np.random.default_rng(seed)
    x = (10.0 ** rng.uniform(-12, 3, (B, T, ld))).astype(np.float32)
    for b in range(B):
        x[b] *= np.float32(10.0 ** (-3 * b))
    kind = rng.integers(0, 40, (B, T, ld))
    x[kind == 0] = 0.0
    x[kind == 1] *= -1.0
    x[kind == 2] = EPS32
    x[kind == 3] = np.nextafter(EPS32, np.float32(0))
    x[kind == 4] = np.nextafter(EPS32, np.float32(1))
    for b in range(B):
        x[b, 0, 0] = 10.0 ** (2.9 - 3 * b)  # every clip's maximum is within 0.1 of its top from frame 0 on
    x[0, T - 1, n_mel // 2] = 1e6
    x[:, :, n_mel:] = 1e30
    return x


def check_log_values(raw, x, n_mel):
    """raw [B][n_mel][T] against melacc x [B][T][ld]: exactly -10 at and below the floor, else float64 log10 within the
    kernel's stated 2e-6 plus half an ulp of the stored float."""
    e = np.transpose(x[:, :, :n_mel], (0, 2, 1))
    floor = ~(e > EPS32)
    assert floor.sum() > 0 and (raw[floor] == np.float32(-10.0)).all(), "floor is not exactly -10"
    ref = np.log10(e[~floor].astype(np.float64))
    err = np.abs(raw[~floor].astype(np.float64) - ref)
    bound = 2e-6 + 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print(f"log_clipmax: max |v - log10| = {err.max():.3e}, at most {(err / bound).max():.3f} of its bound")
    assert (err <= bound).all()


def expected_words(raw, tv):
    """The kernel's own output raw [B][n_mel][T] -> maxima [B][4]: word w takes the 32-frame tiles w, w + 4, ... that
    hold a frame < tv; -inf where no such tile exists."""
    B, _, T = raw.shape
    want = np.full((B, 4), NEG_INF, np.float32)
    for b in range(B):
        for tile in range((min(tv, T) + 31) // 32):
            m = raw[b, :, tile * 32:min(tile * 32 + 32, tv)].max()
            want[b, tile % 4] = max(want[b, tile % 4], m)
    return want


@pytest.mark.parametrize("B,T,n_mel,ld", CLIPMAX_SHAPES)
def test_log_clipmax(eng, B, T, n_mel, ld):
    """Values and partial maxima at tile-edge shapes (T, n_mel on, one past and inside a 32-tile; five frame tiles at
    T = 129, so tile 4 shares word 0 with tile 0) for t_valid in -1, 0, 1, 31, 32, 33, T.  The maxima are compared bit
    for bit with the maximum of the kernel's own output over frames < t_valid, word by word: t_valid 1, 31 and 32 write
    word 0 alone, 33 writes words 0 and 1, 0 writes none; clip 0's largest value sits in frame T - 1 and must show only
    for t_valid = T (or -1); clip 1's maximum is negative; every clip's maximum differs from its neighbours' by ~3."""
    x = clipmax_input(B, T, n_mel, ld, seed=T * 131 + n_mel)
    first = None
    for tv in (-1, 0, 1, 31, 32, 33, T):
        raw, words, maxima = eng.dbg_log_clipmax(x, n_mel, tv)
        if first is None:
            first = raw
            check_log_values(raw, x, n_mel)
        assert np.array_equal(raw.view(np.uint32), first.view(np.uint32)), "t_valid changed the values"
        eff = T if tv < 0 else min(tv, T)
        want = expected_words(raw, eff)
        assert np.array_equal((words != 0), ~np.isneginf(want)), (tv, words)
        assert np.array_equal(maxima.view(np.uint32), want.view(np.uint32)), (tv, maxima, want)
        whole = maxima.max(axis=1)
        if eff > 0:
            assert np.array_equal(whole, raw[:, :, :eff].max(axis=(1, 2)))
            assert (whole[0] > 5.9) == (eff == T)   # the value beyond t_valid shows only once t_valid covers it
            if B > 1:
                assert whole[1] < 0 and (np.abs(np.diff(whole)) > 2).all()
        else:
            assert (words == 0).all() and np.isneginf(whole).all()


def test_log_clipmax_negative_maximum_single_clip(eng):
    """One clip whose every value is below 1 (negative log10) in one tile: the order-preserving bits of a negative
    float must still win over 'never written'."""
    x = clipmax_input(1, 32, 32, 128, seed=5)
    x[:, :, :32] = np.minimum(x[:, :, :32], np.float32(0.5))
    raw, words, maxima = eng.dbg_log_clipmax(x, 32, -1)
    assert (words[0, 1:] == 0).all() and words[0, 0] != 0
    assert maxima[0, 0] == raw.max() and raw.max() < 0


def test_log_clipmax_keeps_nan_out_of_the_maximum(eng):
    """The reference's maximum is `if (mel[i] > mmax)`, which never takes a NaN.  NaN inputs of either sign (a NaN's
    sign bit is arbitrary after a GEMM; with it clear, the order-preserving bits of a NaN lie above every finite
    value's) come out as NaN and take no part in the maximum, in the tile they sit in and in the clip beside them;
    mel_normalize then floors the finite rest against the finite maximum."""
    x = clipmax_input(2, 70, 80, 128, seed=11)
    pos, neg = np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)
    x[0, 5, 7], x[0, 40, 9], x[0, 69, 79] = pos, neg, pos
    x[0, 33, :80] = pos  # a whole frame, as a NaN sample leaves it
    raw, words, maxima = eng.dbg_log_clipmax(x, 80, -1)
    bad = np.isnan(np.transpose(x[:, :, :80], (0, 2, 1)))
    assert np.isnan(raw[bad]).all() and np.isfinite(raw[~bad]).all()
    finite = np.where(bad, NEG_INF, raw)
    print("log_clipmax with NaN inputs: words", [hex(w) for w in words[0]], "maxima", maxima[0])
    assert np.array_equal(maxima.view(np.uint32), expected_words(finite, 70).view(np.uint32))
    out = eng.dbg_mel_normalize(raw, words)
    ref = normalize_ref(raw, finite.max(axis=(1, 2)))
    assert np.isnan(out[bad]).all()
    assert np.array_equal(out[~bad].view(np.uint32), ref[~bad].view(np.uint32))


def test_log_clipmax_refuses_bad_shapes(eng, pkg):
    with pytest.raises(pkg.WtError) as ei:
        eng.dbg_log_clipmax(np.ones((1, 8, 16), np.float32), 17)  # n_mel > ld
    assert ei.value.code == 1
    with pytest.raises(pkg.WtError):
        eng.dbg_log_clipmax(np.ones((1, 8, 16), np.float32), 0)


# ------------------------------------------------------------------------------------------------ mel_normalize ---

def normalize_ref(raw, mmax):
    """The reference's lines 198-212 in float64 (comparisons and arithmetic in double, float stores); mmax [B]."""
    out = np.empty_like(raw)
    for b in range(raw.shape[0]):
        v = raw[b].astype(np.float64)
        floor = np.float64(mmax[b]) - 8.0
        v = np.where(v < floor, np.float64(np.float32(floor)), v)
        out[b] = ((v + 4.0) / 4.0).astype(np.float32)
    return out


@pytest.mark.parametrize("B,T,n_mel", [(3, 70, 80), (1, 33, 33), (2, 129, 80)])
def test_mel_normalize_bit_exact(eng, B, T, n_mel):
    """Clip maxima 2.5 / -1.25 / 0.3 (floors -5.5 / -9.25 / -7.7): values exactly at the floor and one float either
    side of it, clip 0's maximum held in word 3 alone, clip 1's in word 1 beside smaller words, clip 2's in word 0."""
    rng = np.random.default_rng(B * 1000 + T)
    mmax = np.array([2.5, -1.25, 0.3], np.float32)[:B]
    raw = rng.uniform(-10, 1, (B, n_mel, T)).astype(np.float32)
    for b in range(B):
        raw[b] = np.minimum(raw[b] + mmax[b] - 1, mmax[b])
        f = np.float32(np.float64(mmax[b]) - 8.0)
        raw[b, 0, :3] = [f, np.nextafter(f, np.float32(-20)), np.nextafter(f, np.float32(20))]
        raw[b, -1, -1] = mmax[b]
    raw = np.maximum(raw, np.float32(-10.0))
    maxima = np.full((B, 4), NEG_INF, np.float32)
    maxima[0, 3] = mmax[0]
    if B > 1:
        maxima[1] = [-3.0, mmax[1], -9.5, NEG_INF]
    if B > 2:
        maxima[2, 0] = mmax[2]
    out = eng.dbg_mel_normalize(raw, eng.clip_max_words(maxima))
    ref = normalize_ref(raw, mmax)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


def test_t_valid_zero_is_pinned(eng, pkg):
    """A clip with no valid frame (wt_log_mel_spectrogram of fewer than 160 samples returns 80 x 0): log_clipmax
    writes no word, mel_normalize then has no maximum and clamps NOTHING, exactly like the reference, whose maximum
    stays at -1e20 over an empty range: every value is (v + 4) / 4, finite.  In a batch, the clip beside it is
    normalised by its own maximum."""
    x = clipmax_input(2, 40, 80, 128, seed=9)
    raw, words, maxima = eng.dbg_log_clipmax(x, 80, 0)
    assert (words == 0).all()
    mixed = np.zeros((2, 4), np.uint32)
    own = np.float32(raw[1].max())
    mixed[1] = eng.clip_max_words(np.array([NEG_INF, own, NEG_INF, NEG_INF], np.float32))
    out = eng.dbg_mel_normalize(raw, mixed)
    assert np.isfinite(out).all()
    assert np.array_equal(out[0], ((raw[0].astype(np.float64) + 4.0) / 4.0).astype(np.float32))
    assert np.array_equal(out[1], normalize_ref(raw[1:], [own])[0])
    filters = eng.filters()
    assert pkg.log_mel_spectrogram(np.full(100, 0.25, np.float32), filters).shape == (80, 0)


# ------------------------------------------------------------------------------------------------ mel_transpose ---

TRANSPOSE_SHAPES = [(80, 64), (80, 70), (33, 33), (1, 1)]


def transpose_input(B, C, T, seed):
    rng = np.random.default_rng(seed)
    mel = rng.uniform(-1.0, 1.5, (B, C, T)).astype(np.float32)
    flat = mel.reshape(-1)
    # bf16 rounding ties: low half exactly 0x8000 above an even and above an odd upper half, and one step either side
    for i, low in enumerate((0x8000, 0x8000, 0x7FFF, 0x8001)):
        if i < flat.size:
            u = flat[i:i + 1].view(np.uint32)
            u[0] = (u[0] & np.uint32(0xFFFE0000)) | np.uint32((i & 1) << 16) | np.uint32(low)
    return mel


def bf16_rne_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


@pytest.mark.parametrize("C,T", TRANSPOSE_SHAPES)
def test_mel_transpose_fp32(eng, C, T):
    """mel [2][C][T] -> [2][T + 2][C]: rows 1 .. T exact, rows 0 and T + 1 as pre-filled."""
    B = 2
    mel = transpose_input(B, C, T, C * 100 + T)
    fill = np.random.default_rng(1).uniform(100, 200, (B, T + 2, C)).astype(np.float32)
    out = eng.dbg_mel_transpose(mel, fill, planes=0)
    assert np.array_equal(out[:, 1:T + 1].view(np.uint32), np.transpose(mel, (0, 2, 1)).view(np.uint32))
    assert np.array_equal(out[:, [0, T + 1]], fill[:, [0, T + 1]])


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("C,T", TRANSPOSE_SHAPES)
def test_mel_transpose_fp16_planes(eng, C, T, pad):
    """The fp16 plane form at ld = C and ld = C + 1 (the launcher takes any ld >= C): hi = fp16(x * scale), the split
    bound of the module docstring, border rows and padding columns of BOTH planes as pre-filled."""
    B, ld, scale = 2, C + pad, 1024.0
    mel = transpose_input(B, C, T, C * 100 + T)
    fill = np.random.default_rng(2).integers(0x4000, 0x7000, (2, B, T + 2, ld)).astype(np.uint16).view(np.float16)
    out = eng.dbg_mel_transpose(mel, fill, planes=1, scale=scale)
    a = np.transpose(mel, (0, 2, 1)) * np.float32(scale)
    check_split(out[0, :, 1:T + 1, :C], out[1, :, 1:T + 1, :C], a, f"mel_transpose_planes C={C} T={T} ld={ld}")
    keep = np.ones((2, B, T + 2, ld), bool)
    keep[:, :, 1:T + 1, :C] = False
    assert np.array_equal(out.view(np.uint16)[keep], fill.view(np.uint16)[keep])


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("C,T", TRANSPOSE_SHAPES)
def test_mel_transpose_bf16_plane(eng, C, T, pad):
    """The one-plane bf16 form (a single bf16 packed beside a zero, 16-bit store): exactly the round-to-nearest-even
    bf16 of the input, ties included; border rows and padding columns as pre-filled."""
    B, ld = 2, C + pad
    mel = transpose_input(B, C, T, C * 100 + T)
    fill = np.random.default_rng(3).integers(0x4000, 0x7000, (B, T + 2, ld)).astype(np.uint16)
    out = eng.dbg_mel_transpose(mel, fill, planes=2)
    assert np.array_equal(out[:, 1:T + 1, :C], bf16_rne_bits(np.transpose(mel, (0, 2, 1))).reshape(B, T, C))
    keep = np.ones((B, T + 2, ld), bool)
    keep[:, 1:T + 1, :C] = False
    assert np.array_equal(out[keep], fill[keep])


def test_mel_transpose_refuses_bad_shapes(eng, pkg):
    mel = np.zeros((1, 8, 4), np.float32)
    for planes, out in [(0, np.zeros((1, 6, 9), np.float32)),        # the fp32 form has no ld
                        (1, np.zeros((2, 1, 6, 7), np.float16)),     # ld < C
                        (2, np.zeros((1, 6, 7), np.uint16))]:
        with pytest.raises(pkg.WtError) as ei:
            eng.dbg_mel_transpose(mel, out, planes=planes)
        assert ei.value.code == 1


# --------------------------------------------------------------------------- the stages of the real front end ---

@pytest.fixture(scope="module")
def stage_pcm(eng):
    n = eng.dbg_frontend_dims()["samples"]
    pcm = np.zeros((2, n), np.float32)
    s = synth_pcm("speechlike", n, 31).astype(np.float64)
    pcm[0] = (s * (31.9 / np.abs(s).max())).astype(np.float32)   # loud, inside the bound the scales were chosen for
    q = synth_pcm("sweep", 16000, 22).astype(np.float64)
    pcm[1, :16000] = (q * (1e-3 / np.abs(q).max())).astype(np.float32)  # quiet, 1 s, silence behind it
    return pcm


@pytest.fixture(scope="module")
def stages(eng, stage_pcm):
    """ONE call of Engine::logmel over two clips, every intermediate kept (read-only for the tests below)."""
    r = eng.dbg_frontend_stages(stage_pcm)
    for v in r.values():
        v.setflags(write=False)
    return r


def test_stage_planes(eng, stages, stage_pcm):
    """The engine's own pcm_to_planes launch: 480000 samples per clip at stride 480512, the 512 columns behind every
    clip zero (the reference's zero fill past the last sample)."""
    n = stage_pcm.shape[1]
    for b in range(2):
        check_split(stages["hi"][b, :n], stages["lo"][b, :n], stage_pcm[b] * np.float32(PCM_SCALE), f"engine planes clip {b}")
        assert not stages["hi"][b, n:].view(np.uint16).any() and not stages["lo"][b, n:].view(np.uint16).any()
    assert np.array_equal(stages["planes"].astype(np.float64),
                          (stages["hi"].astype(np.float64) + stages["lo"].astype(np.float64)) / PCM_SCALE)


STAGE_ROWS = [0, 1, 2, 3, 97, 98, 99, 100, 101, 710, 1510, 1511, 2996, 2997, 2998, 2999]


def test_stage_power_spectrum(eng, stages):
    """The STFT as the plane GEMM runs it: rows overlap (frame i of clip b = 416 samples from b * 480512 + 160 i),
    power of column pair (2 k, 2 k + 1) at column k.  Reference: |A64 . W64^T|^2 from the returned planes and basis.

    Bar.  test_plane_gemm_plain_and_plane_output holds this kernel's amplitudes to max |X - Xref| < 2e-6 max |Xref|;
    here the maximum is taken over the sampled rows of the same clip, so dX = 2e-6 max |Xref|.  A power is
    P = re^2 + im^2, hence |dP| <= 2 |re| dX + 2 |im| dX + 2 dX^2 (dP = 2 |X| dX, both components, second order kept),
    plus 3 * 2^-24 P for the two products and the sum in fp32.

    Rows: frames 0-3 and 2996-2999 of each clip (2998 and 2999 read past sample 480000 into the zero tail; frame 0 of
    clip 1 is the batch stride), 97-101 (clip 1's sweep ends at sample 16000: 98 and 99 cross into silence), 710 / 1510 / 1511 (clip 0 at its loudest)."""
    d = eng.dbg_frontend_dims()
    T0, n_bins = d["frames"], 201
    W = stages["basis"].astype(np.float64)
    pw = stages["pw"].reshape(2, T0, d["pw_ld"])
    for b in range(2):
        A = np.stack([stages["planes"][b, 160 * i:160 * i + d["dft_k"]] for i in STAGE_ROWS]).astype(np.float64)
        X = A @ W.T
        re, im = X[:, 0:2 * n_bins:2], X[:, 1:2 * n_bins:2]
        P = re * re + im * im
        dX = 2e-6 * np.abs(X).max()
        bound = 2 * (np.abs(re) + np.abs(im)) * dX + 2 * dX * dX + 3 * 2.0 ** -24 * P
        got = pw[b, STAGE_ROWS].astype(np.float64)
        err = np.abs(got[:, :n_bins] - P)
        print(f"power spectrum clip {b}: max |dP| / max P = {err.max() / P.max():.3e}, "
              f"at most {(err / np.maximum(bound, 1e-300)).max():.3f} of the bound")
        assert (err <= bound).all()
        assert (got[:, n_bins:] == 0).all(), "columns past bin 200 meet zero basis rows"
        assert P.max() > 0
    assert (pw[1, 200:] == 0).all(), "clip 1 is silent from frame 100 on: clip 0 must not leak in"


def test_stage_mel_gemm(eng, stages):
    """The full-range mel GEMM (lda = 256 != K = 224) over all 6000 rows against pw64 @ mel_matrix64^T, at the bars
    test_gemm_variants_have_fp32_error holds variant 13 to: max error < 2e-6 of the largest value, and every element
    within 1.5e-6 sum |a||b| (all operands are non-negative here, so that sum is the value itself)."""
    d = eng.dbg_frontend_dims()
    pw = stages["pw"].astype(np.float64)[:, :d["mel_k"]]
    ref = pw @ stages["mel_matrix"].astype(np.float64).T
    got = stages["melacc"].astype(np.float64)
    T0 = d["frames"]
    for b in range(2):
        r, g = ref[b * T0:(b + 1) * T0], got[b * T0:(b + 1) * T0]
        rel = np.abs(g - r).max() / r.max()
        ew = (np.abs(g - r) / np.maximum(r, 1e-300))[r > 0].max()
        print(f"mel GEMM clip {b}: max error / max value = {rel:.3e}, max element-wise relative error = {ew:.3e}")
        assert rel < 2e-6
        assert (np.abs(g - r) <= 1.5e-6 * r).all()
    assert (got[:, 80:] == 0).all()


def test_stage_basis(eng, stages):
    """The windowed DFT basis against float64: row 2 k = c_k hann(n) cos(2 pi k n / 400), row 2 k + 1 = -c_k hann(n)
    sin(2 pi k n / 400), c_k = sqrt 2 for the folded bins 1 .. 199 (sqrt(2) (X_k + conj X_{400-k}) / 2 = sqrt(2) X_k for
    an exact transform; twice its squared magnitude is the reference's |X_k|^2 + |X_{400-k}|^2), 1 for bins 0 and 200.
    Bar: 4 x the largest difference between this construction evaluated in float32 and in float64 (the reference's
    own twiddles are float: its transform is inexact at that order; the whole-path oracle comparison pins the rest)."""
    def build(ft):
        n, k = np.arange(400, dtype=ft)[None, :], np.arange(201, dtype=ft)[:, None]
        hann = (ft(0.5) * (ft(1.0) - np.cos(ft(2.0 * np.pi) * n / ft(400)))).astype(ft)
        ang = (ft(2.0 * np.pi) * (k * n) / ft(400)).astype(ft)
        c = np.where((k >= 1) & (k <= 199), ft(np.sqrt(2.0)), ft(1.0)).astype(ft)
        out = np.zeros((402, 400), ft)
        out[0::2], out[1::2] = c * hann * np.cos(ang), -c * hann * np.sin(ang)
        return out
    ref = build(np.float64)
    bar = 4 * np.abs(build(np.float32).astype(np.float64) - ref).max()
    basis = stages["basis"]
    err = np.abs(basis[:402, :400].astype(np.float64) - ref).max()
    print(f"basis: max |engine - float64| = {err:.3e}, bar (4 x float32 evaluation error) = {bar:.3e}")
    assert err <= bar
    assert not basis[:, 400:].any() and not basis[402:].any()


def test_stage_log_and_normalize(eng, stages):
    """The engine's own log_clipmax and mel_normalize launches at 3000 x 80, ld = 128, judged from THEIR inputs."""
    d = eng.dbg_frontend_dims()
    x = stages["melacc"].reshape(2, d["frames"], d["mel_n"])
    check_log_values(stages["raw"], x, 80)
    want = expected_words(stages["raw"], d["frames"])
    assert np.array_equal(stages["maxima"].view(np.uint32), want.view(np.uint32))
    ref = normalize_ref(stages["raw"], stages["maxima"].max(axis=1))
    assert np.array_equal(stages["mel"].view(np.uint32), ref.view(np.uint32))


def test_stage_final_mel_vs_oracle(eng, orc, stages, stage_pcm):
    """Both clips end to end against the bit-exact restatement of the reference: the loud clip (peak 31.9) is inside
    the bound the fp16 scales were chosen for and gets no allowance."""
    for b in range(2):
        ref = orc.frontend().logmel(stage_pcm[b], eng.filters(), 8)
        err = np.abs(stages["mel"][b] - ref).max()
        print(f"final mel clip {b}: max |delta| = {err:.3e}")
        assert err < MEL_TOL


def test_stage_valid_frames_zero(eng, stage_pcm):
    """Engine::logmel with valid_frames = 0 (what a clip shorter than one hop is): no word written, nothing clamped,
    every value finite."""
    r = eng.dbg_frontend_stages(stage_pcm[:1], valid_frames=0)
    assert (r["words"] == 0).all() and np.isfinite(r["mel"]).all()
    assert np.array_equal(r["mel"], ((r["raw"].astype(np.float64) + 4.0) / 4.0).astype(np.float32))


# ---------------------------------------------------------------------- whole-path behaviour that was unpinned ---

@pytest.fixture(scope="module")
def three_clips(eng):
    n = eng.dbg_frontend_dims()["samples"]
    pcm = np.zeros((3, n), np.float32)
    pcm[0] = synth_pcm("noise", n, 21)
    pcm[1] = synth_pcm("speechlike", n, 31)
    pcm[1, 400000:] = 0.0                     # true silence: the floor of the clip is applied there
    pcm[2, :200000] = synth_pcm("sweep", 200000, 22)
    return pcm


def test_out_of_range_pcm_is_clamped(eng, orc, three_clips):
    """Samples beyond +-32 (ADVICE: out-of-range PCM), +-inf among them: the log-mel is the reference's log-mel of
    np.clip(pcm, -32, 32)."""
    pcm = three_clips.copy()
    pcm[0, 1000:480000:37000] = [40.0, -40.0, 1e30, -1e30, np.inf, -np.inf, 33.0, -32.5, 1e5, -65505.0, 32.001, -np.inf, 64.0][:13]
    pcm[1] *= np.float32(100.0 / np.abs(pcm[1]).max())   # every peak above 32 is cut
    pcm[2, 5000] = np.inf
    mel = eng.logmel_batch(pcm)
    for b in range(3):
        ref = orc.frontend().logmel(np.clip(pcm[b], -PCM_BOUND, PCM_BOUND), eng.filters(), 8)
        err = np.abs(mel[b] - ref).max()
        print(f"clamped clip {b}: max |delta| = {err:.3e}")
        assert np.isfinite(mel[b]).all() and err < MEL_TOL


def nan_frames(index):
    return [i for i in range(3000) if 160 * i <= index < 160 * i + 400]


def test_nan_sample_poisons_only_its_frames(eng, orc, three_clips):
    """One NaN sample at index 80000 of clip 1.  The reference's maximum is `if (mel[i] > mmax)`, which never takes a
    NaN: the frames that hold the sample are NaN, every other frame is floored and normalised as if they were absent.
    The oracle is checked for that first (on the CPU); then the engine: the same frames NaN in all 80 rows, every other
    frame of the clip within MEL_TOL of the oracle, the clips beside it bit-identical to a run without the NaN."""
    pcm = three_clips.copy()
    clean = eng.logmel_batch(pcm)
    pcm[1, 80000] = np.nan
    frames = nan_frames(80000)
    assert frames == [498, 499, 500]
    ref = orc.frontend().logmel(pcm[1], eng.filters(), 8)
    rest = np.ones(3000, bool)
    rest[frames] = False
    assert np.isnan(ref[:, frames]).all() and np.isfinite(ref[:, rest]).all()
    # the oracle kept the NaN out of its maximum: the floor is applied (silence sits exactly 8 decades = 2.0 below it)
    assert ref[:, rest].max() - ref[:, rest].min() == pytest.approx(2.0, abs=1e-6)
    mel = eng.logmel_batch(pcm)
    assert np.isnan(mel[1][:, frames]).all()
    assert np.isfinite(mel[1][:, rest]).all()
    err = np.abs(mel[1][:, rest] - ref[:, rest]).max()
    print(f"NaN clip, frames without the NaN: max |delta| = {err:.3e}")
    assert err < MEL_TOL
    for b in (0, 2):
        assert np.array_equal(mel[b].view(np.uint32), clean[b].view(np.uint32))


def test_nan_sample_through_free_function(pkg, orc, eng):
    """The same through wt_log_mel_spectrogram with a 2 s clip (its maximum runs over 200 valid frames)."""
    pcm = synth_pcm("speechlike", 32000, 33)
    pcm[24000:] = 0.0  # silence that the floor clamps: a NaN taken into the maximum would leave it at -1.5
    pcm[8000] = np.nan
    frames = nan_frames(8000)
    ref = orc.frontend().logmel(pcm, eng.filters(), 4)
    mel = pkg.log_mel_spectrogram(pcm, eng.filters())
    assert mel.shape == ref.shape == (80, 200)
    rest = np.ones(200, bool)
    rest[frames] = False
    assert np.isnan(mel[:, frames]).all() and np.isnan(ref[:, frames]).all()
    assert np.isfinite(mel[:, rest]).all()
    assert np.abs(mel[:, rest] - ref[:, rest]).max() < MEL_TOL


def test_nan_sample_in_a_frames_zero_weight_tail(pkg, orc, eng):
    """Pinned, not wanted: the STFT GEMM reads 416 samples per frame (K is a multiple of 32); the 16 behind the
    reference's 400-sample window meet zero basis entries, and NaN x 0 is NaN.  A NaN at sample s therefore also poisons
    the frame i with 160 i + 400 <= s < 160 i + 416: one frame more than the reference, and only for s mod 160 in
    [80, 96).  Everything else is as in the reference (DESIGN, the front end's clamp / NaN / inf contract)."""
    pcm = synth_pcm("speechlike", 32000, 33)
    pcm[24000:] = 0.0
    pcm[8085] = np.nan
    assert nan_frames(8085) == [49, 50]
    ref = orc.frontend().logmel(pcm, eng.filters(), 4)
    mel = pkg.log_mel_spectrogram(pcm, eng.filters())
    assert [i for i in range(200) if np.isnan(ref[:, i]).any()] == [49, 50]
    assert [i for i in range(200) if np.isnan(mel[:, i]).any()] == [48, 49, 50] and np.isnan(mel[:, 48:51]).all()
    rest = np.ones(200, bool)
    rest[48:51] = False
    assert np.abs(mel[:, rest] - ref[:, rest]).max() < MEL_TOL
