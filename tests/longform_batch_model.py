"""Files of the batched seeking-transcription tests (wt_transcribe_long_batch, wt_engine_set_contexts; DESIGN.md section
22): four recordings on run A's model and options of tests/longform_model.py (P = 78, the micro window of 32 000
samples), transcribed side by side.

On this synthetic model the <|nospeech|> row answers LOUD noise: a window of noise at amplitude 0.005 and above has a
no-speech probability of 1.00 and skip_silence blanks it, a window at 0.002 and below has one near 0 and keeps text — 76
ids behind silence, 30 to 40 behind noise at 0.001.  The files are laid out on that:

  file 0  run A's audio: six windows with skip_silence, two blanked, then its context grows to the truncated 63 ids
  file 1  another seed: a first window at amplitude 0.001 whose 35 kept ids are its context (a fed prompt of 39) under
          the five loud windows behind it
  file 2  shorter than one window: it leaves the batch after the first round
  file 3  six loud windows that skip_silence blanks, so its context stays empty while the others' grow, and a silent tail
          that keeps text

so rounds 3, 4 and 5 hold fed prompts of 67, 39 and 3 ids at once.  The scenario (SCENARIO) runs with
condition_on_previous_text and skip_silence on.  Files 1 to 3 take seed 1, the first of the pool 1 .. 40: with it every
window of every file's reference run under the scenario — tests/longform_ref.py over the CPU oracle — has a decisive
margin (smallest_margin > MARGIN), and none of the files may be set aside, since one indecisive step changes every later
window of its file.  tests/test_longform_batch_reference.py pins that and what the scenario has to exercise; the other
two VARIANTS are run by tests/test_gpu_longform_batch.py on the heads of the files, which asserts their margins itself."""
from __future__ import annotations

import numpy as np

import longform_model as lm
import longform_ref as lr

P, WIN, KEEP, MARGIN = lm.P, lm.WIN, lm.KEEP, lm.MARGIN
STRETCH = lm.STRETCH
LOUD = (0.3, 0.1, 0.5, 0.05, 0.2, 0.4, 0.1, 0.3, 0.1, 0.6, 0.2, 0.05, 0.4, 0.1, 0.3, 0.2)
LOUD_3 = (0.4, 0.1, 0.3, 0.05, 0.5, 0.2, 0.1, 0.3, 0.2, 0.6, 0.05, 0.3, 0.1, 0.4, 0.2, 0.1, 0.5, 0.3, 0.1, 0.2, 0.6, 0.05, 0.3, 0.4)
# (seed, amplitudes per stretch, samples)
FILES = (
    (lm.SEED, lm.AMPS, lm.N_SAMPLES),
    (1, (0.001,) * 4 + LOUD, 20 * STRETCH - 3000),
    (1, (0.002,) * 3, 3 * STRETCH - 3000),
    (1, LOUD_3 + (0.0, 0.0), 26 * STRETCH - 3000),
)
# (condition_on_previous_text, caller context, skip_silence): the scenario first
SCENARIO = (True, (), True)
VARIANTS = (SCENARIO, (False, (), True), (True, lm.CONTEXT, False))


def pcm(f):
    seed, amps, n = FILES[f]
    return lm.pcm(seed, amps, n)


def reference(model, mel_of_file, f, variant=SCENARIO, x=None):
    """longform_ref.transcribe of file f alone: model = an oracle Model of lm.write_model's weights, mel_of_file(f, x,
    seek) = the log-mel of the window of x at that sample."""
    condition, context, skip = variant
    x = pcm(f) if x is None else x
    dec = lr.window_decoder(lm.logits_fn_of(model, lambda seek: mel_of_file(f, x, seek)), len(lm.PROMPT), P, lm.EOT, lm.BEG,
                            lm.NOSP, 50, lm.NO_SPEECH_THRESHOLD / 1000, lm.LOGPROB_THRESHOLD / 1000, skip_silence=skip)
    return lr.transcribe(dec, x.size, WIN, lm.EOT, lm.BEG, lm.PREV, lm.PROMPT, KEEP, context, condition)


def rounds(runs):
    """The batches the loop forms: round r holds window r of every file that has one, as (file, window record)."""
    n = max(len(ws) for ws in runs)
    return [[(f, ws[r]) for f, ws in enumerate(runs) if r < len(ws)] for r in range(n)]
