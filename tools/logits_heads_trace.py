"""Kernel times of the two logits heads (dec_logits_persistent and the int8 head dec_logits_i8) at
whisper-tiny's shape, K = 384, V = 51865, 32 rows, from a kernel trace of the debug taps, both heads alternating:

    rocprofv3 --kernel-trace --stats -d OUT -o heads --output-format csv -- python tools/logits_heads_trace.py run OUT
    python tools/logits_heads_trace.py parse OUT

`run` launches every configuration (head x resident blocks x with / without the logits store) REPS times in turn and
writes the call order to OUT/heads_order.json; `parse` matches the trace's dec_logits kernels to that order and prints
the median, minimum and maximum per configuration, the first two launches of each dropped."""
import csv
import glob
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

CONFIGS = [(head, blocks, y) for blocks in (0, 256) for y in (False, True) for head in ("f16", "i8")]
REPS = 12
mode, out = sys.argv[1], sys.argv[2]

if mode == "run":
    pkg = ge.load_package()
    eng = pkg.Engine(*ge._assets(tempfile.mkdtemp(), "micro", 0), True)
    rng = np.random.default_rng(5)
    K, V, M = 384, 51865, 32
    xin = (rng.standard_normal((M, K)) * 2 + 0.5).astype(np.float32)
    g_, b_ = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    E = (rng.standard_normal((V, K)) / 16).astype(np.float32)
    order = []
    for _ in range(REPS):
        for head, blocks, y in CONFIGS:
            tap = eng.dbg_dec_logits if head == "f16" else eng.dbg_dec_logits_i8
            tap(xin, g_, b_, E, blocks=blocks, want_logits=y)
            order.append([head, blocks, y])
    os.makedirs(out, exist_ok=True)
    json.dump(order, open(os.path.join(out, "heads_order.json"), "w"))
    eng.close()
else:
    order = json.load(open(os.path.join(out, "heads_order.json")))
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))
                 if "dec_logits" in r["Kernel_Name"]]
    rows.sort()
    assert len(rows) == len(order), (len(rows), len(order))
    times = {}
    for (t0, t1, name), cfg in zip(rows, order):
        assert ("dec_logits_i8" in name) == (cfg[0] == "i8"), (name, cfg)
        times.setdefault(tuple(cfg), []).append((t1 - t0) / 1000.0)
    for (head, blocks, y), t in times.items():
        t = np.array(t[2:])
        print(f"{head:3s} blocks {blocks or 512:3d} logits {'written' if y else 'none   '}: median {np.median(t):6.2f} us "
              f"(min {t.min():.2f}, max {t.max():.2f}, n {len(t)})")
