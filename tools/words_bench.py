"""Cost of word-level timestamps: a full-length timestamp decode of synthetic whisper-tiny with
and without option word_timestamps, wall time per call, median of --calls calls, per batch size.

    python tools/words_bench.py --positions 224 --batches 1,32 --configs 1:0,0:0,1:8,1:4

--configs: mode:sub pairs of the alignment pass (wt_dbg_set_alignment): the form of align_scores (0 fused softmax, 1
frame chunks + row kernel) and the most clips per sub-group (0 = what the workspace bound allows).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=224)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--configs", default="1:0")
    args = ap.parse_args()
    pkg = ge.load_package()
    with tempfile.TemporaryDirectory() as tmp:
        prefix, vocab = ge._assets(tmp, "tiny", 0)
        eng = pkg.Engine(prefix, vocab, True)
        eng.set_option("max_positions", args.positions)
        eng.set_option("timestamps", 1)
        eng.set_option("stop_at_eot", 0)  # random weights: every clip runs the whole length
        rng = np.random.default_rng(5)
        for B in (int(b) for b in args.batches.split(",")):
            mel = rng.uniform(-1.0, 1.5, size=(B,) + eng.mel_shape).astype(np.float32)
            res = {"batch": B, "positions": args.positions, "alignment_heads": eng.get_option("alignment_heads")}
            def run():
                times = []
                for _ in range(args.calls + 1):
                    t0 = time.perf_counter()
                    eng.encdec_tokens_full(mel)
                    times.append(1e3 * (time.perf_counter() - t0))
                return round(statistics.median(times[1:]), 2)

            eng.set_option("word_timestamps", 0)
            res["ms_words_off"] = run()
            eng.set_option("word_timestamps", 1)
            for cfg in args.configs.split(","):
                mode, sub = (int(v) for v in cfg.split(":"))
                eng.dbg_set_alignment(mode=mode, sub=sub)
                res[f"ms_words_on_mode{mode}_sub{sub}"] = run()
                res["words"] = int(eng.last_words().size)
            eng.dbg_set_alignment(mode=1, sub=0)
            print(json.dumps(res))
        eng.close()


if __name__ == "__main__":
    main()
