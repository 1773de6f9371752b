"""Host side of the input resampler against tests/resample_ref.py: plan, filter, output length,
refused rates, and the RIFF reader.  No GPU."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_ref as rr  # noqa: E402

RATES = [8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000]


@pytest.mark.parametrize("rate", RATES)
def test_plan_filter_and_length(pkg, rate):
    orig, new, w, K = rr.plan(rate)
    p = pkg.resample_plan(rate)
    assert (p["orig"], p["new"], p["w"], p["K"]) == (orig, new, w, K)
    assert (p["G"] * new) % 16 == 0 and p["Kp"] % 32 == 0 and p["Kp"] >= K + (p["G"] - 1) * orig
    assert p["TM"] % 16 == 0 and p["TM"] >= 16
    h = pkg.resample_filter(rate)
    assert h.shape == (new, K)
    assert np.abs(h - rr.filt(rate)).max() <= 1e-15
    for n in (0, 1, orig - 1, orig, orig + 1):
        assert pkg.resample_len(rate, n) == -(-new * n // orig) == rr.out_len(rate, n)


def test_issue_geometries(pkg):
    got = {r: pkg.resample_plan(r) for r in (48000, 44100, 11025, 8000)}
    assert [(p["orig"], p["new"], p["w"], p["K"]) for p in got.values()] == [(3, 1, 19, 41), (441, 160, 17, 475), (441, 640, 7, 455), (1, 2, 7, 15)]
    assert (got[44100]["G"], got[44100]["Kp"]) == (1, 480) and (got[48000]["G"], got[48000]["Kp"]) == (16, 96)


@pytest.mark.parametrize("rate", [16001, 0])
def test_refused_rates(pkg, rate):
    for call in (lambda: pkg.resample_plan(rate), lambda: pkg.resample_filter(rate), lambda: pkg.resample_len(rate, 5)):
        with pytest.raises(pkg.WtError) as e:
            call()
        assert e.value.code == 1  # WT_ERR_INVALID_ARG


def test_wav_read_walks_the_chunks(pkg, tmp_path):
    x = np.random.default_rng(5).integers(-32768, 32768, size=(1000, 2)).astype(np.int16)
    fmt = struct.pack("<HHIIHH", 1, 2, 44100, 44100 * 4, 4, 16)
    info = b"INFOISFT\x05\x00\x00\x00abcde\x00"  # an odd-sized sub-chunk and its pad byte
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"LIST" + struct.pack("<I", len(info)) + info
    body += b"data" + struct.pack("<I", x.nbytes) + x.tobytes()
    path = tmp_path / "stereo.wav"
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    y, rate = pkg.wav_read(str(path))
    assert rate == 44100 and y.dtype == np.int16 and np.array_equal(y, x)
    with pytest.raises(pkg.WtError):
        pkg.wav_read(str(tmp_path / "missing.wav"))
