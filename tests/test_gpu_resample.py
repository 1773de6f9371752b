"""The input resampler on the GPU (k_resample.hip) against tests/resample_ref.py, and through the
public PCM entry points.  Without the feature none of the symbols used here exists.

The bar of the kernel test, per output j with S[j] = sum_k |h[p][k]| |x[..]| (resample_ref.abs_sum):

    |y - ref| <= (K + 12) 2^-24 S + K 2^-33

Each operand is two fp16 planes, hi = fp16(v s) and lo = fp16(v s - hi) under a power of two s: 22 significand bits, a
relative error of at most 2^-22 per operand wherever lo is a normal number.  The product keeps hi.hi + hi.lo + lo.hi
(each exact in fp32) and drops lo.lo, at most 2^-22 |h| |x|.  Two operand errors and the dropped term are 3 x 2^-22 =
12 x 2^-24 of |h| |x|, summed: 12 x 2^-24 S.  The fp32 accumulation of the K non-zero terms of a row costs at most
K 2^-24 S in any order, because the band's exact zeros add exactly.  Where a lo plane is sub-normal its error is
absolute, half of fp16's smallest step, 2^-25, over the scale: the sample planes carry s = 512 (2^-34 per sample, times
|h| <= 1) and the band planes s >= 2^14 (2^-39, times |x| <= 32), together under 2^-33 per term, K terms.  A kernel that
used the hi planes alone would err by 2^-11 S; the bar is at most 2^-15 S (K <= 475)."""
import os
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_ref as rr  # noqa: E402
from conftest import synth_pcm  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = np.float32(-7.25e11)
# the issue's six rates; 28224 Hz (441 : 250) is the plan whose row of G = 8 blocks does not fit the LDS image: G = 4, one
# row tile per item, and a last column tile that ends in zero columns
RATES = [8000, 11025, 24000, 44100, 48000, 96000, 28224]


@pytest.fixture(scope="module")
def eng(pkg, assets):
    prefix, vocab = assets("tiny")
    e = pkg.Engine(prefix, vocab, True)
    yield e
    e.close()


def run_dev(eng, x, rate, batch=1, n=None, guard=GUARD):
    """resample_batch_dev on x [batch][in_stride(, channels)]: rows of n_out floats, the guards around every row checked"""
    x = np.ascontiguousarray(x)
    fmt = 1 if x.dtype == np.int16 else 0
    ch = x.shape[2] if x.ndim == 3 else 1
    n, stride_in = x.shape[1] if n is None else n, x.shape[1]  # n < the stride: junk behind every clip's frames
    n_out = rr.out_len(rate, n) if rate != 16000 else n
    row = guard + n_out + guard
    host = np.full((batch, row), PATTERN, np.float32)
    d_in, d_out = eng.device_array(x), eng.device_array(host)
    try:
        eng.resample_batch_dev(d_in.data_ptr(), fmt, ch, rate, n, batch, stride_in, d_out.data_ptr() + 4 * guard, row)
        got = d_out.download()
    finally:
        d_in.free()
        d_out.free()
    assert np.array_equal(got[:, :guard].view(np.uint32), host[:, :guard].view(np.uint32)), "front guard written"
    assert np.array_equal(got[:, guard + n_out:].view(np.uint32), host[:, guard + n_out:].view(np.uint32)), "rear guard written"
    return got[:, guard:guard + n_out]


@pytest.mark.parametrize("rate", RATES)
def test_kernel_against_float64(eng, pkg, rate):
    p = pkg.resample_plan(rate)
    K, T, row = p["K"], p["TM"] * p["G"] * p["orig"], p["G"] * p["orig"]
    rng = np.random.default_rng(rate)
    cases = [(n, 1.0, GUARD) for n in (1, p["w"], row - 1, T, T + 1, 3 * T + row // 2 + 1)] + [(T + 1, 31.0, 61)]
    worst = 0.0
    for n, amp, guard in cases:  # guard 61: the output rows start off a 16-byte boundary (scalar stores)
        x = rng.standard_normal(n)
        x = (amp * x / np.abs(x).max()).astype(np.float32)
        y = run_dev(eng, x[None, :], rate, guard=guard)[0]
        bar = (K + 12) * 2.0 ** -24 * rr.abs_sum(x, rate) + K * 2.0 ** -33
        err = np.abs(y.astype(np.float64) - rr.resample(x, rate))
        ratio = float((err / bar).max())
        worst = max(worst, ratio)
        print(f"resample {rate} Hz n={n} amp={amp}: worst |err| / bar = {ratio:.4f}")
        assert ratio <= 1.0, (rate, n, amp, ratio)
    print(f"resample {rate} Hz: worst ratio to the bar {worst:.4f}")


def test_batch_clips_do_not_bleed(eng, pkg):
    p = pkg.resample_plan(48000)
    n = p["TM"] * p["G"] * p["orig"] + 5
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, size=(3, n + 777)).astype(np.float32)  # junk behind every clip's n frames
    got = run_dev(eng, x, 48000, batch=3, n=n)
    for b in range(3):
        alone = run_dev(eng, x[b:b + 1, :n], 48000)[0]
        assert np.array_equal(got[b].view(np.uint32), alone.view(np.uint32)), b


def test_formats_and_downmix(eng):
    rng = np.random.default_rng(4)
    v = rng.integers(-32768, 32768, size=5000).astype(np.int16)
    f = v.astype(np.float32) / np.float32(32768.0)
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
    mono = eng.resample(f, 44100)
    assert same(eng.resample(v, 44100), mono)
    assert same(eng.resample(np.stack([f, f], 1), 44100), mono)
    assert same(eng.resample(np.stack([v, v], 1), 44100), mono)
    assert not np.any(eng.resample(np.stack([f, -f], 1), 44100))
    g = rng.uniform(-1, 1, size=(5000, 2)).astype(np.float32)
    assert same(eng.resample(g, 16000), (g[:, 0] + g[:, 1]) * np.float32(0.5))
    assert same(run_dev(eng, g[None], 16000)[0], (g[:, 0] + g[:, 1]) * np.float32(0.5))


@pytest.mark.parametrize("rate", [11025, 48000])
def test_a_sine_is_a_sine(eng, rate):
    x = np.sin(2 * np.pi * 1000.0 * np.arange(rate // 10) / rate).astype(np.float32)
    y = eng.resample(x, rate)
    want = np.sin(2 * np.pi * 1000.0 * np.arange(y.size) / 16000.0)
    d = float(np.abs(y - want)[100:-100].max())
    print(f"1 kHz at {rate} Hz: max |y - sine| = {d:.3e}")
    assert y.size == 1600 and d <= 2e-3


def test_public_path(eng, pkg, tmp_path):
    """48 kHz stereo int16 under the input options == the defaults on the resampled recording"""
    def stereo48(seconds, seed):
        m = synth_pcm("speechlike", 16000 * seconds * 3, seed)  # the generator's tones land at a third of their pitch
        return np.stack([np.round(m * 30000), np.round(m * 15000)], 1).astype(np.int16)

    def with_input(on):
        for key, val in (("input_sample_rate", 48000), ("input_channels", 2), ("input_format", pkg.WT_PCM_S16)):
            eng.set_option(key, val if on else {"input_sample_rate": 16000, "input_channels": 1, "input_format": 0}[key])

    x48 = stereo48(30, 11)
    x16 = eng.resample(x48, 48000)
    assert x16.size == 480000
    before = eng.transcribe(x16)
    lang16 = eng.detect_language_pcm(x16)
    wav = str(tmp_path / "x16.wav")
    with wave.open(wav, "wb") as f:
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(16000)
        f.writeframes(np.round(x16 * 32767).astype(np.int16).tobytes())
    from_file = eng.transcribe(wav)
    with_input(True)
    assert eng.transcribe(x48) == before
    assert eng.detect_language_pcm(x48) == lang16
    assert eng.transcribe(wav) == from_file  # a path's samples come from the legacy reader: the options do not describe them
    with_input(False)
    long48 = stereo48(70, 12)
    long16 = eng.resample(long48, 48000)
    # (no text carried from window to window: 32 positions hold the prompt alone)
    for key, val in (("max_positions", 32), ("timestamps", 1), ("seek", 1), ("condition_on_previous_text", 0)):
        eng.set_option(key, val)
    text16 = eng.transcribe_long(long16)
    win16 = eng.last_windows()
    with_input(True)
    assert eng.transcribe_long(long48) == text16
    assert eng.last_windows().tobytes() == win16.tobytes() and len(win16) >= 3
    assert eng.transcribe_long_batch([long48, x48])[0] == text16
    with_input(False)
    for key, val in (("seek", 0), ("timestamps", 0), ("max_positions", 0), ("condition_on_previous_text", 1)):
        eng.set_option(key, val)
    assert eng.transcribe(x16) == before
