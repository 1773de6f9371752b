"""Kernel times of the encoder-block GEMMs in both forms (gemm_planes on fp16 planes, and the int8 pair enc_quant_rows_i8
+ enc_gemm_i8) at whisper-tiny's four shapes, M = 48 000 rows (32 clips), from a kernel trace of the
debug taps, both forms alternating:

    rocprofv3 --kernel-trace --stats -d OUT -o gemms --output-format csv -- python tools/enc_gemm_i8_trace.py run OUT
    python tools/enc_gemm_i8_trace.py parse OUT

`run` launches every (shape, form) REPS times in turn and writes the call order to OUT/gemms_order.json; `parse` matches
the trace's kernels to that order and prints the median, minimum and maximum per configuration, the first two launches
of each dropped.  The int8 column is the quantise launch plus the GEMM launch: the quantiser is part of the price."""
import csv
import glob
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

D, M, REPS = 384, 48000, 12
# name, N, K, the plane GEMM's epilogue flags, the int8 epilogue, the quantiser's source
SHAPES = [("qkv", 3 * D, D, 1, 1, "ln"), ("out", D, D, 5, 0, "planes"), ("fc1", 4 * D, D, 3, 2, "ln"), ("fc2", D, 4 * D, 5, 0, "f32")]
mode, out = sys.argv[1], sys.argv[2]

if mode == "run":
    pkg = ge.load_package()
    eng = pkg.Engine(*ge._assets(tempfile.mkdtemp(), "micro", 0), True)
    rng = np.random.default_rng(5)
    order = []
    for name, N, K, epi_p, epi_8, src in SHAPES:
        X = rng.standard_normal((M, K), dtype=np.float32)
        W, bias = (rng.standard_normal((N, K)) / 16).astype(np.float32), rng.standard_normal(N).astype(np.float32)
        R = rng.standard_normal((M, N), dtype=np.float32) if epi_8 == 0 else None
        g_, b_ = (rng.standard_normal(K).astype(np.float32) for _ in range(2)) if src == "ln" else (None, None)
        for _ in range(REPS):
            eng.dbg_gemm_planes(X, W, bias, R=R, epi=epi_p)
            qx, sx = eng.dbg_enc_quant_rows_i8(X, src, scale=0.125, ln_g=g_, ln_b=b_)
            eng.dbg_enc_gemm_i8(qx, sx, W, bias, R=R, epi=epi_8)
            order += [[name, "f16"], [name, "i8 quant"], [name, "i8 gemm"]]
    os.makedirs(out, exist_ok=True)
    json.dump(order, open(os.path.join(out, "gemms_order.json"), "w"))
    eng.close()
else:
    order = json.load(open(os.path.join(out, "gemms_order.json")))
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))
                 if any(k in r["Kernel_Name"] for k in ("gemm_planes", "enc_quant", "enc_gemm_i8"))]
    rows.sort()
    assert len(rows) == len(order), (len(rows), len(order))
    times = {}
    for (t0, t1, name), cfg in zip(rows, order):
        want = {"f16": "gemm_planes", "i8 quant": "enc_quant", "i8 gemm": "enc_gemm_i8"}[cfg[1]]
        assert want in name, (name, cfg)
        times.setdefault(tuple(cfg), []).append((t1 - t0) / 1000.0)
    for name in dict.fromkeys(c[0] for c in order):
        t = {form: np.array(times[(name, form)][2:]) for form in ("f16", "i8 quant", "i8 gemm")}
        t["i8 both"] = t["i8 quant"] + t["i8 gemm"]
        print(f"{name:4s} " + "  ".join(f"{form}: median {np.median(v):7.1f} us ({v.min():.1f} .. {v.max():.1f})" for form, v in t.items()))
