#!/usr/bin/env python3
"""The kernels of option full_bf16_all on one MI355X, through the debug taps: the ragged forms of
self_attention_long (H = 6, cap 448, 125 rows, starts 0 .. 4 cycled, slots 32, 128 and 447) in fp32 and bf16, and
align_scores (H = 6, T = 1500, 32 clips x 4 positions, every head of the layer, mode 1: the chunked kernel;
align_softmax_rows, the same in both modes, is not counted) in fp32 and bf16; the two forms alternating, `--reps`
launches each.  Run it under the profiler in a run of its own and hand the kernel trace to --report:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/full_bf16_all_profile.py --run
  python tools/full_bf16_all_profile.py --report OUT

The taps launch one kernel of a kind per call, so the dispatches in the trace are the calls in order."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, H, CAP = 125, 6, 448
SLOTS = (32, 128, 447)
ALIGN = (32, 1500, 4)  # clips, frames, positions


def plan(reps):
    calls = [("long_ragged", slot, bf) for slot in SLOTS for _ in range(reps) for bf in (False, True)]
    calls += [("align_scores", ALIGN, bf) for _ in range(reps) for bf in (False, True)]
    return calls


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def run(reps):
    sys.path.insert(0, ROOT)
    import tempfile

    import __graft_entry__ as ge
    pkg = ge.load_package()
    with tempfile.TemporaryDirectory() as tmp:
        prefix, vocab = ge._assets(tmp, "micro", 0)
        eng = pkg.Engine(prefix, vocab, True)
        rng = np.random.default_rng(0)
        d = 64 * H
        kc = bf16_round(rng.standard_normal((ROWS, CAP, d)).astype(np.float32))  # (the same operands for both forms)
        vc = bf16_round(rng.standard_normal((ROWS, CAP, d)).astype(np.float32))
        qkv = rng.standard_normal((ROWS, 3 * d)).astype(np.float32)
        starts = (np.arange(ROWS) % 5).astype(np.int32)
        B, T, n_pos = ALIGN
        E = bf16_round(rng.standard_normal((B, T, d)).astype(np.float32))
        qp = (rng.standard_normal((n_pos, B, H * d)) * (13.0 / np.sqrt(d))).astype(np.float32)
        F = np.full(B, T, np.int32)
        W = np.zeros((B, H, n_pos, T), np.float32)
        for kind, arg, bf in plan(reps):
            if kind == "long_ragged":
                eng.dbg_self_attention_long_ragged(qkv, kc, vc, arg, starts, CAP, bf16=bf)
            else:
                eng.dbg_align_scores(qp, E, np.arange(H), np.arange(H), F, W, 0, 1, bf16=bf)
        eng.close()


def report(out_dir, reps):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {out_dir}")
    rows = {"long_ragged": [], "align_scores": []}
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"]
                kind = "long_ragged" if "self_attention_long" in name else "align_scores" if "align_scores" in name else None
                if kind:
                    rows[kind].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    times = {}
    for kind in rows:
        calls = [c for c in plan(reps) if c[0] == kind]
        got = sorted(rows[kind])
        if len(got) != len(calls):
            raise SystemExit(f"{len(got)} dispatches of {kind} in the trace, {len(calls)} calls planned")
        for call, (_, ns) in zip(calls, got):
            times.setdefault(call, []).append(ns)
    for (kind, arg, bf), t in times.items():
        t = np.asarray(t[1:], np.float64)  # (the first launch of a shape loads its code)
        print(json.dumps({"kernel": kind, "shape": arg, "form": "bf16" if bf else "fp32", "launches": int(t.size),
                          "median_us": float(np.median(t)) / 1e3, "min_us": float(t.min()) / 1e3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--report", metavar="DIR")
    ap.add_argument("--reps", type=int, default=8)
    a = ap.parse_args()
    if a.run:
        run(a.reps)
    if a.report:
        report(a.report, a.reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
