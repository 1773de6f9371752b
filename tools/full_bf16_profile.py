#!/usr/bin/env python3
"""The fp32 and bf16 forms of self_attention_long, its gathered form and self_attention_prefill
on one MI355X, through the debug taps: H = 6, cap 448; the long and gathered kernels over 125 rows at positions 32, 128
and 447 (the gathered form under a random-parent table), the prefill kernel at the shapes of the table of section 20;
fp32 and bf16 alternating, `--reps` launches each.  Run it under the profiler in a run of its own and hand the kernel
trace to --report:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/full_bf16_profile.py --run
  python tools/full_bf16_profile.py --report OUT

The taps launch one kernel per call, so the dispatches of the two kernels in the trace are the calls in order.  Bytes of
a launch, e = 4 or 2 bytes per cache element: long / gathered — K and V rows 0 .. pos - 1 read and row pos written, 64 e
per (row, head, position, k|v), plus the qkv and out rows (fp32) and pos table bytes per (row, head) block; prefill —
qkv read, cache rows < pos0 read once, new rows and the output written."""
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
POSITIONS = (32, 128, 447)
PREFILL = ((1, 0, 128), (1, 128, 100), (32, 0, 4), (32, 224, 4))  # (B, pos0, np)


def plan(reps):
    calls = [("long", pos, bf) for pos in POSITIONS for _ in range(reps) for bf in (False, True)]
    calls += [("gather", pos, bf) for pos in POSITIONS for _ in range(reps) for bf in (False, True)]
    calls += [("prefill", shape, bf) for shape in PREFILL for _ in range(reps) for bf in (False, True)]
    return calls


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


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
        table = rng.integers(0, ROWS, size=(ROWS, CAP)).astype(np.uint8)
        pre = {s: rng.standard_normal((s[2] * s[0], 3 * d)).astype(np.float32) for s in PREFILL}
        for kind, arg, bf in plan(reps):
            if kind == "long":
                eng.dbg_self_attention_long(qkv, kc, vc, arg, bf16=bf)
            elif kind == "gather":
                eng.dbg_self_attention_long_gather(qkv, kc, vc, arg, table, bf16=bf)
            else:
                B, pos0, n = arg
                eng.dbg_self_attention_prefill(pre[arg], kc[:B], vc[:B], pos0, n, bf16=bf)
        eng.close()


def nbytes(kind, arg, bf):
    e = 2 if bf else 4
    if kind == "prefill":
        B, pos0, n = arg
        return B * H * 64 * (n * 3 * 4 + 2 * pos0 * e + 2 * n * e + n * 4)
    table = arg if kind == "gather" else 0
    return ROWS * H * (2 * (arg + 1) * 64 * e + 4 * 256 + table)


def report(out_dir, reps):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {out_dir}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "self_attention_long" in r["Kernel_Name"] or "self_attention_prefill" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    calls = plan(reps)
    if len(rows) != len(calls):
        raise SystemExit(f"{len(rows)} dispatches of the two kernels in the trace, {len(calls)} calls planned")
    times = {}
    for call, (_, ns) in zip(calls, rows):
        times.setdefault(call, []).append(ns)
    for call, t in times.items():
        kind, arg, bf = call
        t = np.asarray(t[1:], np.float64)  # (the first launch of a shape loads its code)
        b = nbytes(kind, arg, bf)
        print(json.dumps({"kernel": kind, "shape": arg, "form": "bf16" if bf else "fp32", "launches": int(t.size),
                          "median_us": float(np.median(t)) / 1e3, "min_us": float(t.min()) / 1e3, "bytes": b,
                          "TB_per_s": b / float(np.median(t)) / 1e3}))


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
