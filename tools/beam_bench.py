#!/usr/bin/env python3
"""Beam-search costs on one MI355X, synthetic tiny weights:
  * single-clip transcribe latency (wt_transcribe_pcm) at beam_size 1 and K;
  * audio-sec/s of wt_encdec_tokens_batch_dev at beam_size K with 25 and 64 clips (and greedy beside it).
With --max-positions P the batch cases run the full-length chains instead: full-length beam
search (full_beam = 1) beside full-length greedy decoding at the same P, ms per call and per decoder step; the
synthetic weights never emit EOT, so every step runs.  With --suppress-ab every full-length case runs four times, the
suppression lists cleared and option suppress_default = 1 alternating.  With --bf16 every case runs
in the bf16 storage mode (with --max-positions: option full_bf16).
Every GPU step runs in a child process of its own under a time limit; the parent only collects the JSON lines.

  python tools/beam_bench.py [--beam 5] [--iters 10] [--only CASE] [--max-positions P [--suppress-ab]] [--bf16]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(case: str, beam: int, iters: int, tmp: str, max_positions: int = 0, suppress: int = 0, bf16: bool = False) -> dict:
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    prefix, vocab = ge._assets(tmp, "tiny", 0)
    eng = pkg.Engine(prefix, vocab, True)
    eng.set_option("beam_size", beam)
    if bf16:
        eng.set_option("bf16", 1)
        if max_positions:
            eng.set_option("full_bf16", 1)
    if max_positions:
        eng.set_option("max_positions", max_positions)
        eng.set_option("full_beam", 1)
        eng.set_option("suppress_default", suppress)
    rng = np.random.default_rng(1234)
    if case == "latency":
        pcm = (0.1 * rng.standard_normal(eng.pcm_len)).astype(np.float32)
        for _ in range(3):
            eng.transcribe(pcm)
        t = []
        for _ in range(iters):
            t0 = time.perf_counter()
            eng.transcribe(pcm)
            t.append(time.perf_counter() - t0)
        out = {"case": "transcribe_latency_ms", "beam_size": beam, "median": 1e3 * float(np.median(t)),
               "min": 1e3 * float(np.min(t))}
    else:
        batch = int(case)
        mel = rng.uniform(-1.0, 1.5, size=(batch,) + eng.mel_shape).astype(np.float32)
        d = ctypes_dev(pkg, eng, mel)
        run = (lambda: eng.encdec_tokens_full_dev(d, batch)) if max_positions else (lambda: eng.encdec_tokens_batch_dev(d, batch))
        for _ in range(3):
            run()
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        dt = (time.perf_counter() - t0) / iters
        tm = eng.timings()
        out = {"case": "encdec_tokens_full_batch_dev" if max_positions else "encdec_tokens_batch_dev", "beam_size": beam,
               "batch": batch, "ms_per_call": 1e3 * dt, "audio_sec_per_s": batch * 30.0 / dt, "decoder_ms": tm.decoder_ms}
        if max_positions:
            steps = int(tm.decoder_steps)
            out.update(max_positions=max_positions, decoder_steps=steps, decoder_ms_per_step=tm.decoder_ms / max(steps, 1),
                       suppress_default=suppress, suppress_ids=eng.get_option("suppress_ids"),
                       suppress_first_ids=eng.get_option("suppress_first_ids"))
    out["bf16"] = int(bf16)
    eng.close()
    return out


def ctypes_dev(pkg, eng, a):
    import ctypes
    p = ctypes.c_void_p()
    L = pkg.lib()
    assert L.wt_device_alloc(eng.handle, ctypes.c_size_t(a.nbytes), ctypes.byref(p)) == 0
    assert L.wt_device_upload(eng.handle, p, 0, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes)) == 0
    return p.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--only", default=None, help="latency, 25 or 64")
    ap.add_argument("--max-positions", type=int, default=0, help="full-length chains over this many positions (0: 31-position chains)")
    ap.add_argument("--suppress-ab", action="store_true", help="with --max-positions: lists cleared / suppress_default, alternating")
    ap.add_argument("--bf16", action="store_true", help="the bf16 storage mode (with --max-positions: option full_bf16)")
    ap.add_argument("--suppress", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--child", nargs=3, metavar=("CASE", "BEAM", "TMP"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child[0], int(a.child[1]), a.iters, a.child[2], a.max_positions, a.suppress, a.bf16)))
        return 0
    runs = [("latency", 1), ("latency", a.beam), ("25", 1), ("25", a.beam), ("64", 1), ("64", a.beam)]
    if a.only:
        runs = [r for r in runs if r[0] == a.only]
    runs = [r + (0,) for r in runs]
    if a.suppress_ab and a.max_positions:
        runs = [(c, b, s) for c, b, _ in runs if c != "latency" for s in (0, 1, 0, 1)]
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        for case, beam, suppress in runs:
            cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--max-positions", str(a.max_positions),
                   "--suppress", str(suppress)] + (["--bf16"] if a.bf16 else []) + ["--child", case, str(beam), tmp]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(json.dumps({"case": case, "beam_size": beam, "error": "timeout"}))
                return 124
            if p.returncode != 0:
                print(json.dumps({"case": case, "beam_size": beam, "error": p.returncode, "stderr": p.stderr[-2000:]}))
                return 1  # nothing more on the GPU after a failed step
            line = p.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            results.append(json.loads(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
