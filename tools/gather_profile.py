#!/usr/bin/env python3
"""Cost of the gathered form of self_attention_long on one MI355X, through the debug taps:
H = 6, cap 448, 125 rows, positions 32, 128 and 447; a random-parent table against the identity table against the
ungathered kernel, alternating, `--reps` launches each.  Run it under the profiler in a run of its own and hand the
kernel trace to --report:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/gather_profile.py --run
  python tools/gather_profile.py --report OUT

The tap launches one kernel per call, so the dispatches of self_attention_long in the trace are the calls in order.
Bytes of a launch: K and V rows 0 .. pos - 1 read and row pos written, 256 B per (row, head, position, k|v), plus the
qkv and out rows; the table adds pos bytes per (row, head) block."""
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
VARIANTS = ("random", "identity", "ungathered")


def plan(reps):
    return [(pos, v) for pos in POSITIONS for _ in range(reps) for v in VARIANTS]


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
        kc = rng.standard_normal((ROWS, CAP, d)).astype(np.float32)
        vc = rng.standard_normal((ROWS, CAP, d)).astype(np.float32)
        qkv = rng.standard_normal((ROWS, 3 * d)).astype(np.float32)
        tables = {"random": rng.integers(0, ROWS, size=(ROWS, CAP)).astype(np.uint8),
                  "identity": np.repeat(np.arange(ROWS, dtype=np.uint8)[:, None], CAP, axis=1)}
        for pos, v in plan(reps):
            if v == "ungathered":
                eng.dbg_self_attention_long(qkv, kc, vc, pos)
            else:
                eng.dbg_self_attention_long_gather(qkv, kc, vc, pos, tables[v])
        eng.close()


def report(out_dir, reps):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {out_dir}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "self_attention_long" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    calls = plan(reps)
    if len(rows) != len(calls):
        raise SystemExit(f"{len(rows)} dispatches of self_attention_long in the trace, {len(calls)} calls planned")
    times = {}
    for (pos, v), (_, ns) in zip(calls, rows):
        times.setdefault((pos, v), []).append(ns)
    for pos in POSITIONS:
        nbytes = ROWS * H * (2 * (pos + 1) * 256 + 4 * 256)
        for v in VARIANTS:
            t = np.asarray(times[(pos, v)][1:], np.float64)  # (the first launch of a shape loads its code)
            print(json.dumps({"pos": pos, "variant": v, "launches": int(t.size), "median_us": float(np.median(t)) / 1e3,
                              "min_us": float(t.min()) / 1e3, "max_us": float(t.max()) / 1e3, "bytes": nbytes,
                              "GB_per_s": nbytes / float(np.median(t))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--report", metavar="DIR")
    ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    if a.run:
        run(a.reps)
    if a.report:
        report(a.report, a.reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
