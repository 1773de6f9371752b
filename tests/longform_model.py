"""Model and audio of the seeking-transcription tests (options seek and condition_on_previous_text, the context of
wt_engine_set_context): the timestamp model of tests/ts_model.py with only the first 101 timestamp
rows scaled — the micro window is 200 frames = 32 000 samples = 100 ticks, so the loud timestamps stay inside it (ticks
101 .. 1500 keep the quiet rows' scale and are practically never chosen; the loop clamps one that is) — and with the
<|nospeech|> row scaled as tests/scores_model.py does, which changes no id under the timestamp rules.

Two runs make the scenario: A (TS_GAIN, the whole audio, the default max_initial_timestamp) takes the seek rule's pairs
and no-pair-behind-a-timestamp branches, truncates the context and differs between the settings of
condition_on_previous_text; B (TS_GAIN_B, max_initial_timestamp 0, the head of the audio) takes the single-ending-timestamp
and the open-segment branches.

The audio is several windows of seeded noise, every stretch of STRETCH samples with an amplitude of its own, one of them
silent.  Seed, gains, amplitudes and thresholds were chosen on the CPU; tests/test_longform_reference.py pins what the
oracle front end + decoder + tests/longform_ref.py give on them."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import full_model  # noqa: E402
import scores_model  # noqa: E402
import ts_model  # noqa: E402

EOT, BEG, NOSP = ts_model.EOT, ts_model.BEG, scores_model.NOSP
PREV = 50361                      # <|startofprev|> of the multilingual vocabulary
PROMPT = ts_model.PROMPT          # [sot, <|de|>, transcribe]
N_TEXT_CTX = ts_model.N_TEXT_CTX  # 128: the engine keeps 63 context ids, the longest fed prompt has 67
KEEP = N_TEXT_CTX // 2 - 1
P = 78                            # positions fed: 11 behind the longest fed prompt, and references that take seconds
WIN = 32000                       # samples of a micro window
WIN_TICKS = WIN // 320
LOUD_TICKS = WIN_TICKS + 1        # timestamp rows scaled: ticks 0 .. 100
TS_GAIN = 1500.0                  # 101 loud rows need more than ts_model's 1300 over 1501 for their sum to compete
NOSP_GAIN = scores_model.NOSP_GAIN
MARGIN = ts_model.MARGIN
SEED = 5
STRETCH = 8000                    # samples per amplitude
AMPS = (0.1, 0.3, 0.02, 0.5, 0.1, 0.05, 0.4, 0.2, 0.0, 0.0, 0.0, 0.0, 0.3, 0.1, 0.6, 0.02, 0.2, 0.1, 0.4, 0.05,
        0.3)
N_SAMPLES = len(AMPS) * STRETCH - 3000   # the last window is a partial one
# the second run: the same model with the timestamp rows a little louder, the first timestamp held at <|0.00|>
# (max_initial_timestamp = 0) and the first 14 stretches of the audio.  Its first window runs to the position cap behind a
# single closing timestamp and a later one holds no timestamp but <|0.00|>: the two branches the first run never takes
TS_GAIN_B, MAX_INITIAL_B = 1600.0, 0
AMPS_B = AMPS[:14]
N_SAMPLES_B = len(AMPS_B) * STRETCH - 3000
CONTEXT = (11, 222, 333, 44, 555)        # a caller's context: it seeds the first window
NO_SPEECH_THRESHOLD, LOGPROB_THRESHOLD = 600, 0  # thousandths (skip_silence): a window is blanked on its no-speech probability alone


def write_model(src_wtw, dst_wtw, ts_gain=TS_GAIN, rich=ts_model.RICH):
    from wtw import read_wtw, write_wtw
    full_model.write_eot_rich(src_wtw, dst_wtw, rich[0], rich[1], rich[2], n_text_ctx=N_TEXT_CTX)
    dims, t = read_wtw(dst_wtw)
    t = {k: np.array(v) for k, v in t.items()}
    t["decoder.token_embedding.weight"][BEG:BEG + LOUD_TICKS] *= np.float32(ts_gain)
    t["decoder.token_embedding.weight"][NOSP] *= np.float32(NOSP_GAIN)
    write_wtw(dst_wtw, dims, t)


def pcm(seed=SEED, amps=AMPS, n_samples=N_SAMPLES):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(len(amps) * STRETCH).astype(np.float32)
    x *= np.repeat(np.asarray(amps, np.float32), STRETCH)
    return np.ascontiguousarray(x[:n_samples])


def window(x, seek, win=WIN):
    """x[seek : seek + win], zero-padded."""
    out = np.zeros(win, np.float32)
    part = x[seek:seek + win]
    out[: part.size] = part
    return out


def logits_fn_of(model, mel_of, max_pos=P):
    """logits_fn_of(w, seek) for longform_ref.window_decoder: the CPU oracle's decoder behind mel_of(seek), the log-mel
    [80][200] of the window at that sample (the oracle front end's on the CPU, the engine's own on the GPU)."""
    enc = {}  # the encoder output of a window, shared by every run over the same audio

    def fn(w, seek):
        if seek not in enc:
            enc[seek] = model.encode(mel_of(seek))
        return ts_model.logits_fn(model, enc[seek], max_pos)
    return fn

