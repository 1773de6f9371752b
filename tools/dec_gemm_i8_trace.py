"""Kernel times of the decoder-block GEMMs in both forms (dec_gemm on fp16 planes and the int8 dec_gemm_i8, DESIGN.md
section 38) at whisper-tiny's five shapes, 32 rows, from a kernel trace of the debug taps, both forms alternating:

    rocprofv3 --kernel-trace --stats -d OUT -o gemms --output-format csv -- python tools/dec_gemm_i8_trace.py run OUT
    python tools/dec_gemm_i8_trace.py parse OUT

`run` launches every (shape, form) REPS times in turn and writes the call order to OUT/gemms_order.json; `parse` matches
the trace's dec_gemm kernels to that order and prints the median, minimum and maximum per configuration, the first two
launches of each dropped.  fc2 on fp16 planes is the engine's default form, split over K (two halves in one launch)."""
import csv
import glob
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

D, M, REPS = 384, 32, 12
SHAPES = [("qkv", 3 * D, D, "ln"), ("out", D, D, "resid"), ("cross_out", D, D, "resid"), ("fc1", 4 * D, D, "ln_gelu"),
          ("fc2", D, 4 * D, "resid")]
mode, out = sys.argv[1], sys.argv[2]

if mode == "run":
    pkg = ge.load_package()
    eng = pkg.Engine(*ge._assets(tempfile.mkdtemp(), "micro", 0), True)
    rng = np.random.default_rng(5)
    g_, b_ = rng.standard_normal(D).astype(np.float32), rng.standard_normal(D).astype(np.float32)
    ops = {}
    for name, N, K, kind in SHAPES:
        ops[name] = ((rng.standard_normal((M, K)) * 2 + 0.5).astype(np.float32), (rng.standard_normal((N, K)) / 16).astype(np.float32),
                     rng.standard_normal(N).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32))
    order = []
    for _ in range(REPS):
        for name, N, K, kind in SHAPES:
            X, W, bias, R = ops[name]
            if kind == "resid":
                if name == "fc2":
                    eng.dbg_dec_gemm_ksplit(X, W, bias, R)
                else:
                    eng.dbg_dec_gemm(X, W, bias, mode=2, R=R)
                eng.dbg_dec_gemm_i8(W, bias, X=X, R=R, epi=0)
            else:
                eng.dbg_dec_ln_gemm_rows(W, bias, g_, b_, xin=X, gelu=kind == "ln_gelu")
                eng.dbg_dec_gemm_i8(W, bias, xin=X, ln_g=g_, ln_b=b_, epi=2 if kind == "ln_gelu" else 1)
            order += [[name, "f16"], [name, "i8"]]
    os.makedirs(out, exist_ok=True)
    json.dump(order, open(os.path.join(out, "gemms_order.json"), "w"))
    eng.close()
else:
    order = json.load(open(os.path.join(out, "gemms_order.json")))
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))
                 if "dec_gemm" in r["Kernel_Name"]]
    rows.sort()
    assert len(rows) == len(order), (len(rows), len(order))
    times = {}
    for (t0, t1, name), cfg in zip(rows, order):
        assert ("dec_gemm_i8" in name) == (cfg[1] == "i8"), (name, cfg)
        times.setdefault(tuple(cfg), []).append((t1 - t0) / 1000.0)
    for (name, form), t in times.items():
        t = np.array(t[2:])
        print(f"{name:9s} {form:3s}: median {np.median(t):6.2f} us (min {t.min():.2f}, max {t.max():.2f}, n {len(t)})")
