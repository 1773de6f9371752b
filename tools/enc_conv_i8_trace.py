"""Kernel times of the encoder's two convolutions in both forms (gemm_planes on fp16 planes, and the int8 stem kernels
clip_absmax_f32 + enc_conv*_i8) at whisper-tiny's shapes, 32 clips, from a kernel trace of the
debug taps, both forms alternating:

    rocprofv3 --kernel-trace --stats -d OUT -o convs --output-format csv -- python tools/enc_conv_i8_trace.py run OUT
    python tools/enc_conv_i8_trace.py parse OUT

`run` launches every (shape, form) REPS times in turn and writes the call order to OUT/convs_order.json; `parse` matches
the trace's kernels to that order and prints the median, minimum and maximum per configuration, the first two launches
of each dropped.  The plane GEMM runs on a dense matrix of the convolution's M x K (the same products; the engine's
implicit addressing reads a third of those A bytes), with bias + GELU."""
import csv
import glob
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

B, D, REPS = 32, 384, 12
SHAPES = [("conv1", 1, 3000, 80, 1), ("conv2", 2, 1500, D, 2)]  # name, stride, T_out, C_in, the int8 epilogue
KERNELS = {"f16": "gemm_planes", "i8 max": "clip_absmax", "i8 conv": "enc_conv"}
mode, out = sys.argv[1], sys.argv[2]

if mode == "run":
    pkg = ge.load_package()
    eng = pkg.Engine(*ge._assets(tempfile.mkdtemp(), "micro", 0), True)
    rng = np.random.default_rng(5)
    order = []
    for name, stride, T_out, C_in, epi in SHAPES:
        X = rng.standard_normal((B, stride * T_out, C_in), dtype=np.float32)
        W, bias = (rng.standard_normal((D, C_in, 3)) / 16).astype(np.float32), rng.standard_normal(D).astype(np.float32)
        pos = rng.standard_normal((T_out, D), dtype=np.float32)
        KP = (3 * C_in + 31) // 32 * 32  # the plane kernels take K in steps of 32: zero columns, as the engine's table has
        A, W2 = np.zeros((B * T_out, KP), np.float32), np.zeros((D, KP), np.float32)
        A[:, :3 * C_in] = rng.standard_normal((B * T_out, 3 * C_in), dtype=np.float32)
        W2[:, :3 * C_in] = W.transpose(0, 2, 1).reshape(D, -1)
        for _ in range(REPS):
            eng.dbg_gemm_planes(A, W2, bias, epi=3)
            eng.dbg_enc_conv_i8(X, W, bias, stride=stride, epi=epi, pos=pos)
            order += [[name, "f16"], [name, "i8 max"], [name, "i8 conv"]]
    os.makedirs(out, exist_ok=True)
    json.dump(order, open(os.path.join(out, "convs_order.json"), "w"))
    eng.close()
else:
    order = json.load(open(os.path.join(out, "convs_order.json")))
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))
                 if any(k in r["Kernel_Name"] for k in KERNELS.values())]
    rows.sort()
    assert len(rows) == len(order), (len(rows), len(order))
    times = {}
    for (t0, t1, name), cfg in zip(rows, order):
        assert KERNELS[cfg[1]] in name, (name, cfg)
        times.setdefault(tuple(cfg), []).append((t1 - t0) / 1000.0)
    for name in dict.fromkeys(c[0] for c in order):
        t = {form: np.array(times[(name, form)][2:]) for form in KERNELS}
        print(f"{name:5s} " + "  ".join(f"{form}: median {np.median(v):7.1f} us ({v.min():.1f} .. {v.max():.1f})" for form, v in t.items()))
