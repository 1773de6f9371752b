#!/usr/bin/env python3
"""bench.py — audio-sec/s of the EncDec hot path (BASELINE.json metric) on N MI355X.

One "step" = one pass of the hot path over one batch of synthetic input per rank:
device-resident mel [32][80][3000] fp32 (configs[1]: whisper-tiny, batch 32 x 30 s) ->
encoder -> cross-KV -> 30 decoder positions / 27 greedy argmax steps -> token ids on the
host (wt_encdec_tokens_batch_dev), then (N > 1) one RCCL all_gather of the fixed-stride id
records.  Inputs are already in HBM when the timed region starts.

  python bench.py --gpus 1 --steps 20 --warmup 3
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
      --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0: the headline (metric, value, unit, ms_per_step, dtype, config).
`--full` adds what takes instrumentation or runs of its own: per-kernel event timers and rooflines,
stage times, the isolated passes, the CPU baseline and the extra legs (fp32 MFMA, front end,
outlier / trained-like weights, configs[3]).  `--dump-outputs DIR` writes the ids and id counts of
the last timed step as DIR/*.npy (float64).  `--dry-run-gloo` exercises only the sharding + gather
plumbing on CPU (world_size-2 gloo test in tests/test_distributed.py).
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BATCH_PER_GPU = 32
CLIP_SECONDS = 30.0
MEL_SEED = 1234
ID_STRIDE = 32  # int64 ids per clip record (wt_capi.h WT_MAX_IDS)
GATHER_EVERY = 8  # batches per all_gather of id records (N > 1)
FORCE_COLLECTIVES = False  # --rehearse-nccl: run the RCCL collectives of the N > 1 path on one rank
PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak (v_mfma_f32_32x32x16_bf16, 32 cycles)
PEAK_HBM_GBPS = 8000.0


# ---------------------------------------------------------------- sharding / gather ---

def shard_range(rank: int, world: int, total: int):
    """Contiguous clip range of `rank`: clips [r*B/R, (r+1)*B/R)."""
    per = total // world
    rem = total % world
    lo = rank * per + min(rank, rem)
    return lo, lo + per + (1 if rank < rem else 0)


def pack_records(ids: np.ndarray, n: np.ndarray) -> np.ndarray:
    """Fixed-stride record per clip: 32 int64 ids followed by the id count."""
    rec = np.zeros((ids.shape[0], ID_STRIDE + 1), np.int64)
    rec[:, :ID_STRIDE] = ids
    rec[:, ID_STRIDE] = n
    return rec


def gather_records(rec_tensor, world: int):
    """The path's only collective: all_gather of the per-rank id records (RCCL over xGMI on
    GPUs; gloo in the CPU rehearsal).  Returns [world * B][33]."""
    import torch
    import torch.distributed as dist
    if world == 1 and not FORCE_COLLECTIVES:
        return rec_tensor
    out = [torch.empty_like(rec_tensor) for _ in range(world)]
    dist.all_gather(out, rec_tensor)
    return torch.cat(out, dim=0)


def synthetic_mel(lo: int, hi: int, shape) -> np.ndarray:
    """mel ~ U(-1, 1.5), one independent stream per GLOBAL clip index, so a clip's content
    does not depend on how the batch is sharded."""
    out = np.empty((hi - lo,) + tuple(shape), np.float32)
    for i, g in enumerate(range(lo, hi)):
        out[i] = np.random.default_rng([MEL_SEED, g]).uniform(-1.0, 1.5, size=shape).astype(np.float32)
    return out


# ------------------------------------------------------------------------ dry run ---

def dry_run_gloo(args) -> None:
    """CPU rehearsal of the N > 1 plumbing: same sharding, same records, same collective, with
    a deterministic stand-in for the engine (ids derived from the clip's global index)."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    total = world * args.batch
    lo, hi = shard_range(rank, world, total)
    ids = np.zeros((hi - lo, ID_STRIDE), np.int64)
    n = np.zeros(hi - lo, np.int32)
    for i, g in enumerate(range(lo, hi)):
        n[i] = 5 + g % 27
        ids[i, : n[i]] = (np.arange(n[i]) * 7 + g * 13) % 51865
    rec = gather_records(torch.from_numpy(pack_records(ids, n)), world).numpy()
    ok = rec.shape == (total, ID_STRIDE + 1)
    for g in range(total):
        cnt = 5 + g % 27
        ok = ok and rec[g, ID_STRIDE] == cnt and np.array_equal(rec[g, :cnt], (np.arange(cnt) * 7 + g * 13) % 51865)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"dry_run": True, "world": world, "clips": int(total), "ok": bool(ok)}))
    if not ok:
        sys.exit(1)


# -------------------------------------------------------------------- cpu baseline ---

def cpu_baseline(prefix: str, mel: np.ndarray, prompt, eot: int) -> dict:
    """TEST-INFRASTRUCTURE leg: the oracle (CPU port of the same path) timed on this host's
    cores over a bounded sample of the same workload.  Reported beside the GPU number; never
    the thing measured as `value`."""
    import __graft_entry__ as ge
    orc = ge.load_oracle()
    cores = min(os.cpu_count() or 1, 16)
    model = orc.Model(prefix + ".wtw")
    sample = mel[: min(2 * cores, mel.shape[0])]  # 32 clips on a 16-core box: the whole GPU batch
    t0 = time.perf_counter()
    ids_c, n_c = model.encdec_batch(sample, prompt, 30, eot, False, True, n_threads=cores)
    t_cached = time.perf_counter() - t0
    # reference-faithful structure (whisper.cpp:367-375): no KV cache, whole prefix per step
    few = sample[: max(1, cores // 2)]
    t0 = time.perf_counter()
    model.encdec_batch(few, prompt, 30, eot, False, False, n_threads=cores)
    t_nocache = time.perf_counter() - t0
    model.close()
    return {
        "value": round(sample.shape[0] * CLIP_SECONDS / t_cached, 2),
        "unit": "audio-sec/s",
        "cores": cores,
        "kind": "port",
        "sample": f"{sample.shape[0]} clips of the same synthetic batch, KV-cached oracle, one clip per thread "
                  f"({t_cached:.1f} s); reference-structure (no KV cache) on {few.shape[0]} clips: "
                  f"{few.shape[0] * CLIP_SECONDS / t_nocache:.2f} audio-sec/s ({t_nocache:.1f} s)",
        "nocache_value": round(few.shape[0] * CLIP_SECONDS / t_nocache, 2),
        "reference_tflite_cpu_path": "unavailable (no TFLite runtime / .tflite model in this environment)",
        "ids": ids_c,
        "n": n_c,
    }



# ----------------------------------------------------------------------- rooflines ---

def rooflines(ks, steps):
    """per kernel class: achieved = algorithmic FLOPs (bytes) / summed launch durations (HIP event pairs on the
    stream the kernels run on).  Plane / split kernels spend 3 (two fp16 planes per operand, the default) or 6 (three
    bf16 planes: the fp32-storage fall-back form) 16-bit MFMA FLOPs per algorithmic fp32 FLOP: their MFMA ceiling in
    algorithmic FLOP/s is the dense f16/bf16 peak / products; fp32-MFMA kernels are priced against the fp32 MFMA peak."""
    det = {}
    for name, v in ks.items():
        if v["launches"] == 0 or v["ms"] <= 0:
            continue
        mfma = v["flops"] > 0
        ach = (v["flops"] / 1e12 if mfma else v["bytes"] / 1e9) / (v["ms"] * 1e-3)
        bf = "bf16_planes" in name or name == "encoder_attention_bf16"  # bf16 storage mode: one product
        planes = "planes" in name and not bf  # the default kernels: operands stored as two fp16 planes
        split = mfma and ("split" in name or planes or bf)
        products = 1 if bf else 3 if planes else 6
        peak = (round(PEAK_BF16_MFMA_TFLOPS / products, 1) if split else PEAK_F32_MFMA_TFLOPS) if mfma else PEAK_HBM_GBPS
        det[name] = {"bound": "mfma" if mfma else "hbm", "achieved": round(ach, 2), "peak": peak,
                     "unit": "TFLOP/s" if mfma else "GB/s", "frac": round(ach / peak, 4),
                     "avg_launch_us": round(1e3 * v["ms"] / v["launches"], 2),
                     "launches_per_step": v["launches"] // steps,
                     "ms_per_step": round(v["ms"] / steps, 4)}
        if split:
            det[name].update({"peak_is": f"dense f16/bf16 MFMA peak 2500 TFLOP/s / {products} plane products",
                              "executed_16bit_tflops": round(products * ach, 1),
                              "vs_fp32_mfma_peak": round(ach / PEAK_F32_MFMA_TFLOPS, 4)})
    return det


def add_stats(acc, ks):
    for name, v in ks.items():
        a = acc.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
        for k in a:
            a[k] += v[k]


def pipeline_run(eng, ptr, batch, k, depth, on_collect=None, tail=2):
    """k pipelined passes of the hot path over the device-resident batch at `ptr`; returns the last (ids, n)"""
    in_flight, out = 0, None
    for i in range(k):
        if tail and k - i == tail:
            eng.set_option("last_batches", tail)  # the job's last batches drain as one decoder chain per batch
        eng.pipeline_submit_dev(ptr, batch)
        in_flight += 1
        if in_flight == depth:
            out = eng.pipeline_collect()
            in_flight -= 1
            if on_collect:
                on_collect()
    while in_flight:
        out = eng.pipeline_collect()
        in_flight -= 1
        if on_collect:
            on_collect()
    return out


def timed_leg(eng, ptr, batch, steps, warm, depth, sync):
    """steps timed pipelined passes after `warm` untimed ones; per-launch kernel stats of the sampled passes"""
    pipeline_run(eng, ptr, batch, warm, depth)
    sync()
    ks, sampled = {}, [0]

    def acc():
        st = eng.kernel_stats()
        if any(v["launches"] for v in st.values()):
            sampled[0] += 1
        add_stats(ks, st)

    t0 = time.perf_counter()
    ids, n = pipeline_run(eng, ptr, batch, steps, depth, acc)
    sync()
    dt = time.perf_counter() - t0
    return dt, ids, n, rooflines(ks, max(1, sampled[0]))


def traffic_from_profile(dom, bf16, known_names):
    """HBM-side bytes per launch of kernel class `dom` from the committed rocprofv3 --pmc summary (separate
    FETCH_SIZE / WRITE_SIZE passes, tools/pmc_traffic.py).  A summary that was recorded for kernels this library no
    longer launches is refused (traffic null) instead of being quoted stale."""
    for tf in (("r04_c4_pmc_traffic.json", "r03_c4_pmc_traffic.json") if bf16 else ("r04_pmc_traffic.json", "r03_pmc_traffic.json")):
        try:
            with open(os.path.join(ROOT, "profiles", tf)) as f:
                t = json.load(f)
            recorded = t["kernel_class"].split()[0]
            per = [k.split("<")[0] for k in t.get("per_kernel", {}) if k.startswith(recorded)]
            if recorded != dom or recorded not in known_names or not per:
                continue
            return int(t["traffic_bytes_per_launch"]), "profiles/" + tf
        except (OSError, KeyError, ValueError, IndexError):
            continue
    return None, "no committed --pmc summary names kernel class " + str(dom)


# ---------------------------------------------------------------------------- main ---

def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=BATCH_PER_GPU, help="clips per GPU")
    ap.add_argument("--arch", default="tiny")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="synchronous steps (encoder then decoder) instead of the two-deep pipeline")
    ap.add_argument("--depth", type=int, default=None, choices=tuple(range(1, 25)),
                    help="batches in flight (pipelined mode); default 10, or 3 x --dec-group + 4 from three batches per chain on")
    ap.add_argument("--dec-group", type=int, default=None, choices=(1, 2, 3, 4),
                    help="consecutive steps' batches that share one decoder chain (engine default 2; 1 = a chain per batch)")
    ap.add_argument("--tail", type=int, default=2, choices=(0, 1, 2, 3, 4),
                    help="announce the last N batches of every run of steps to the engine (option last_batches: one decoder "
                         "chain per batch while the pipeline drains); 0 = never")
    ap.add_argument("--attn-variant", type=int, default=None, choices=(0, 1, 4))
    ap.add_argument("--cross-chunks", type=int, default=None, choices=(1, 2, 4, 8))
    ap.add_argument("--cross-absorb", type=int, default=None, choices=(0, 1),
                    help="0 = round 2's cross-KV cache instead of the absorbed cross-attention (default 1)")
    ap.add_argument("--abs-chunks", type=int, default=None, help="key chunks per clip of the absorbed cross-attention (0 = automatic)")
    ap.add_argument("--no-fp32-leg", action="store_true", help="skip the extra fp32-MFMA-only measurement")
    ap.add_argument("--no-graphs", action="store_true", help="launch the decoder eagerly instead of replaying its hipGraph")
    ap.add_argument("--gemm-variant", type=int, default=None, help="encoder GEMM tile variant (k_gemm.hip)")
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"),
                    help="collective backend for N > 1 (gloo only to rehearse the multi-rank flow on a 1-GPU box)")
    ap.add_argument("--single-device", action="store_true",
                    help="rehearsal: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--dry-run-gloo", action="store_true")
    ap.add_argument("--bf16", action="store_true",
                    help="bf16 storage mode (BASELINE.json configs[3]: bf16 weights / activations / KV caches, fp32 "
                         "accumulate); quote it with --arch base --batch 64")
    ap.add_argument("--kernel-timers", type=int, default=None,
                    help="event pairs around every encoder launch on every N-th pass (0 = off; engine default 1)")
    ap.add_argument("--emit-ids", action="store_true", help="add a CRC of every step's ids and the gathered record count to the line")
    ap.add_argument("--report-maps", action="store_true", help="add the libamdhip64 files this process has mapped to the line")
    ap.add_argument("--rehearse-nccl", action="store_true",
                    help="single rank: create the RCCL communicator and run the N > 1 collectives anyway")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: kernel event timers and rooflines, stage times, "
                         "isolated passes, CPU baseline and the extra legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's ids and id counts as DIR/<name>.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dry_run_gloo:
        dry_run_gloo(args)
        return

    import __graft_entry__ as ge

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    if args.single_device:
        local_rank = 0
    global FORCE_COLLECTIVES
    FORCE_COLLECTIVES = bool(args.rehearse_nccl) and world == 1
    if FORCE_COLLECTIVES:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
    # One HIP runtime in the measured path: every device buffer the engine touches is allocated by the ENGINE
    # (wt_device_alloc: the ROCm libamdhip64 the product links), never by torch, whose wheel bundles a HIP runtime of its
    # own.  torch is imported only where a collective is needed (N > 1, --rehearse-nccl); its tensors — the id records of
    # the all_gather — never meet an engine pointer: ids leave the engine as host arrays.  At N = 1 the process maps one
    # libamdhip64.
    torch = dist = None
    if world > 1 or FORCE_COLLECTIVES:
        import torch
        import torch.distributed as dist
        if args.backend == "nccl":
            if not torch.cuda.is_available():
                raise SystemExit("bench.py needs an MI355X: there is no CPU fallback for the engine")
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    pkg = ge.load_package()
    tmp = tempfile.mkdtemp(prefix=f"wt_bench_r{rank}_")
    prefix, vocab = ge._assets(tmp, args.arch, 0)
    eng = pkg.Engine(prefix, vocab, True, device_id=local_rank)  # fails loudly (WT_ERR_DEVICE) without a gfx950 GPU
    if args.attn_variant is not None:
        eng.set_option("attn_variant", args.attn_variant)
    if args.cross_chunks:
        eng.set_option("cross_chunks", args.cross_chunks)
    if args.cross_absorb is not None:
        eng.set_option("cross_absorb", args.cross_absorb)
    if args.abs_chunks is not None:
        eng.set_option("abs_chunks", args.abs_chunks)
    if os.environ.get("WT_NO_PAIR") or args.dec_group == 1:
        eng.set_option("dec_pair", 0)
    elif args.dec_group:
        eng.set_option("dec_group", args.dec_group)
    if args.depth is None:
        args.depth = 10 if (args.dec_group or 2) <= 2 else 3 * args.dec_group + 4
    if args.no_graphs:
        eng.set_option("use_graphs", 0)
    if args.gemm_variant is not None:
        eng.set_option("gemm_variant", args.gemm_variant)
    if args.bf16:
        eng.set_option("bf16", 1)
    # --full: per-launch HIP event pairs on every 4th encoder pass of the timed region (an event pair per launch on every
    # pass costs ~1 % of the pipeline period); the headline alone runs without them
    eng.set_option("kernel_timers", (4 if args.full else 0) if args.kernel_timers is None else args.kernel_timers)
    eng.set_option("stop_at_eot", 0)  # full-length decode: 30 positions, 27 argmax steps
    B = args.batch
    lo, hi = shard_range(rank, world, world * B)
    mel_host = synthetic_mel(lo, hi, eng.mel_shape)
    d_mel = eng.device_array(mel_host)  # resident in HBM before the timed region
    eng.device_synchronize()

    pipelined = not args.no_pipeline
    host = {"submit_s": 0.0, "submits": 0}  # host time spent enqueueing (launch-bound check)

    # N > 1: the id records of GATHER_EVERY consecutive batches travel in one all_gather (fewer, larger
    # collectives: an RCCL kernel per batch would sit in a hardware queue next to a decoder chain and
    # couple the ranks batch by batch).  Every record is gathered inside the timed region.
    pending = []
    gathered = {"rec": None, "collectives": 0, "records": 0, "crc": 0, "digest": 0}

    def flush_gather():
        if not pending:
            return
        rec = np.concatenate(pending, axis=0)
        pending.clear()
        if world > 1 or FORCE_COLLECTIVES:
            t = torch.from_numpy(rec)
            rec = gather_records(t.cuda() if args.backend == "nccl" else t, world).cpu().numpy()
            gathered["collectives"] += 1
        gathered["rec"] = rec
        gathered["records"] += int(rec.shape[0])
        if args.emit_ids:
            import zlib
            rec = np.ascontiguousarray(rec)
            gathered["crc"] = zlib.crc32(rec.tobytes(), gathered["crc"])
            # order-independent digest of the records (a sum of per-record CRCs): equal for any split of the same global
            # clips over ranks and batches
            gathered["digest"] = (gathered["digest"] + sum(zlib.crc32(r.tobytes()) for r in rec)) & 0xFFFFFFFFFFFF

    def finish(ids, n):
        pending.append(pack_records(ids, n))
        if len(pending) >= GATHER_EVERY:
            flush_gather()
        return ids, n, gathered["rec"]

    def step():
        return finish(*eng.encdec_tokens_batch_dev(d_mel.data_ptr(), B))

    def run_steps(k, on_step=None):
        """k passes of the hot path.  Pipelined: up to --depth batches are in flight (encoder on
        one HIP stream, decoders rotating over three more); all k batches start and
        finish inside the call."""
        out = None
        if not pipelined:
            for _ in range(k):
                out = step()
                if on_step:
                    on_step()
            flush_gather()
            return out[0], out[1], gathered["rec"]
        in_flight = 0
        for i in range(k):
            if args.tail and k - i == args.tail:
                # the job's last batches: one decoder chain per batch (option last_batches, DESIGN section 5 "drain")
                eng.set_option("last_batches", args.tail)
            t_h = time.perf_counter()
            eng.pipeline_submit_dev(d_mel.data_ptr(), B)
            host["submit_s"] += time.perf_counter() - t_h
            host["submits"] += 1
            in_flight += 1
            if in_flight == args.depth:
                out = finish(*eng.pipeline_collect())
                in_flight -= 1
                if on_step:
                    on_step()
        while in_flight:
            out = finish(*eng.pipeline_collect())
            in_flight -= 1
            if on_step:
                on_step()
        flush_gather()
        return out[0], out[1], gathered["rec"]

    # engine initialisation, outside warm-up and timing like the weight upload: the first batch sets kernel
    # attributes and captures the decoder's hipGraphs (one per pipeline slot)
    run_steps(1)
    if args.warmup:
        run_steps(args.warmup)

    def fence():
        if world > 1 or FORCE_COLLECTIVES:
            dist.barrier()
            if args.backend == "nccl":
                torch.cuda.synchronize()
        eng_now.device_synchronize()  # hipDeviceSynchronize() in the engine's runtime: the device is idle

    class _Live:  # the engine fence() synchronises (the extra-engine legs swap it)
        def device_synchronize(self):
            (self.e or eng).device_synchronize()
        e = None
    eng_now = _Live()

    stage = {"encoder_ms": 0.0, "cross_kv_ms": 0.0, "decoder_ms": 0.0}
    kstats = {}
    sampled = {"steps": 0}  # steps whose encoder pass carried per-launch event pairs (option kernel_timers)
    def accumulate():
        t = eng.timings()
        for k in stage:
            stage[k] += getattr(t, k)
        ks = eng.kernel_stats()
        if any(v["launches"] for v in ks.values()):
            sampled["steps"] += 1
        for name, v in ks.items():
            acc = kstats.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            for k in acc:
                acc[k] += v[k]

    gathered.update(collectives=0, records=0, crc=0, digest=0)  # count the timed region only
    fence()
    t0 = time.perf_counter()
    ids, n, rec = run_steps(args.steps, accumulate if args.full else None)
    fence()
    elapsed = time.perf_counter() - t0
    timed = dict(gathered)
    if world > 1 or FORCE_COLLECTIVES:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if args.backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step: the ids ([clip][32], zero after the count) and the
        # id counts of this rank's batch; at N > 1 also the gathered records of that step ([global clip][32 ids + count])
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "ids.npy"), np.asarray(ids, np.float64))
        np.save(os.path.join(args.dump_outputs, "n_ids.npy"), np.asarray(n, np.float64))
        if world > 1:
            last = rec.reshape(world, -1, B, ID_STRIDE + 1)[:, -1].reshape(world * B, ID_STRIDE + 1)
            np.save(os.path.join(args.dump_outputs, "records.npy"), last.astype(np.float64))

    # the same pipeline with every ENCODER contraction on the fp32 MFMA instruction (reported beside
    # the headline, outside the timed region, so the effect of the plane kernels is visible)
    fp32_leg = None
    if args.full and pipelined and args.gemm_variant is None and args.attn_variant is None and not args.no_fp32_leg and not args.bf16:
        eng.set_option("gemm_variant", 0)
        eng.set_option("attn_variant", 0)
        run_steps(3)
        fence()
        t1 = time.perf_counter()
        ids32, n32, _ = run_steps(10)
        fence()
        dt = time.perf_counter() - t1
        fp32_leg = {"value": round(world * B * 10 * CLIP_SECONDS / dt, 1), "unit": "audio-sec/s", "steps": 10,
                    "ms_per_step": round(1e3 * dt / 10, 3),
                    "ids_match_split_path": bool(np.array_equal(ids32, ids) and np.array_equal(n32, n)),
                    "what": "ENCODER on gemm_variant=0 (gemm_f32_tile), attn_variant=0 (encoder_attention_f32): "
                            "v_mfma_f32_32x32x2_f32 only; the decoder keeps its fp16-plane GEMMs (not an end-to-end "
                            "IEEE-fp32 line: the leg prices the encoder's contraction form)"}
        # and on the bf16 three-plane split kernels (full fp32 operand range)
        eng.set_option("gemm_variant", 16)
        eng.set_option("attn_variant", 1)
        run_steps(3)
        fence()
        t1 = time.perf_counter()
        ids3, n3, _ = run_steps(20)
        fence()
        dt = time.perf_counter() - t1
        fp32_leg["bf16x3_split"] = {"value": round(world * B * 20 * CLIP_SECONDS / dt, 1), "steps": 20,
                                    "ms_per_step": round(1e3 * dt / 20, 3),
                                    "ids_match": bool(np.array_equal(ids3, ids) and np.array_equal(n3, n)),
                                    "what": "gemm_variant=16, attn_variant=1: three bf16 planes, six products"}
        eng.set_option("gemm_variant", -1)
        eng.set_option("attn_variant", 4)

    # second number of SURVEY 8(d): the same pipeline fed with device-resident PCM, i.e. with the log-mel
    # front end (whisper.cpp:109-216) inside every step; PCM ~ N(0, 0.1^2) clipped to [-1, 1]
    with_frontend = None
    if args.full and pipelined and not args.no_fp32_leg and not args.bf16:
        pcm_host = np.clip(np.random.default_rng([MEL_SEED, 7]).normal(0.0, 0.1, size=(B, eng.pcm_len)), -1, 1).astype(np.float32)
        d_pcm = eng.device_array(pcm_host)
        eng.device_synchronize()

        def run_pcm(k):
            in_flight = 0
            for _ in range(k):
                eng.pipeline_submit_pcm_dev(d_pcm.data_ptr(), B)
                in_flight += 1
                if in_flight == args.depth:
                    eng.pipeline_collect()
                    in_flight -= 1
            while in_flight:
                eng.pipeline_collect()
                in_flight -= 1

        d_mel2 = eng.device_array(np.zeros_like(mel_host))
        eng.logmel_batch_dev(d_pcm.data_ptr(), B, d_mel2.data_ptr())
        t1 = time.perf_counter()
        for _ in range(5):
            eng.logmel_batch_dev(d_pcm.data_ptr(), B, d_mel2.data_ptr())
        logmel_ms = 1e3 * (time.perf_counter() - t1) / 5
        d_mel2.free()
        run_pcm(5)
        fence()
        t1 = time.perf_counter()
        run_pcm(40)
        fence()
        dt = time.perf_counter() - t1
        with_frontend = {"value": round(world * B * 40 * CLIP_SECONDS / dt, 1), "unit": "audio-sec/s", "steps": 40,
                         "ms_per_step": round(1e3 * dt / 40, 3), "logmel_ms_per_batch_alone": round(logmel_ms, 3),
                         "input": "PCM [32][480000] resident in HBM, N(0, 0.1^2) clipped"}
        d_pcm.free()

    legs_ok = args.full and pipelined and world == 1 and not args.no_fp32_leg and not args.bf16 and args.arch == "tiny" \
        and args.gemm_variant is None and args.attn_variant is None

    # What trained-like weight statistics cost: the same workload on weights whose layer-0 value projection has one
    # channel 10^4 x larger (and the out-projection column that much smaller).  The load-time slack check gives THAT
    # attention and out-projection the full-range three-plane kernels; every other contraction keeps the plane kernels.
    # (both extra-engine legs run after the main engine is closed: the runtime spreads ALL live streams of the process over
    # four hardware queues, and a second engine's encoder stream next to the first one's idle streams can land on the
    # queue of its own decoder chains — measured 82 k instead of 107 k audio-sec/s on the configs[3] leg)
    def run_outlier_leg():
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from wtw import adversarial_weights
        adv = os.path.join(tmp, "tiny-outlier")
        adversarial_weights(prefix + ".wtw", adv + ".wtw", ln_gain=1.0, heavy=False, v_row_scale=1.0e4)
        e2 = pkg.Engine(adv, vocab, True, device_id=local_rank)
        e2.set_option("stop_at_eot", 0)
        e2.set_option("kernel_timers", 4)
        eng_now.e = e2
        dt, _, n2, det2 = timed_leg(e2, d_mel.data_ptr(), B, 40, 12, args.depth, fence)
        outlier_leg = {"value": round(B * 40 * CLIP_SECONDS / dt, 1), "unit": "audio-sec/s", "steps": 40,
                       "ms_per_step": round(1e3 * dt / 40, 3), "f16_fallbacks": int(e2.get_option("f16_fallbacks")),
                       "launches_per_step": {k: v["launches_per_step"] for k, v in det2.items()},
                       "all_clips_decoded": bool((n2 == 31).all()),
                       "weights": "tools/wtw.py adversarial_weights(v_row_scale=1e4): layer 0 attention + out-projection "
                                  "fall back to three bf16 planes (gemm_split16_tile / encoder_attention_split), the "
                                  "other contractions stay on the plane kernels"}
        e2.close()
        return outlier_leg

    # The same on weights with trained-checkpoint statistics in EVERY layer (tools/wtw.py trained_like_weights: log-normal
    # LayerNorm gains with outlier channels, heavy-tailed rows, two massive residual channels): how many of the 23
    # contractions the load-time check takes off the fp16-plane kernels, and what that costs.
    def run_trained_like_leg():
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from wtw import trained_like_weights

        def one(tag, what, **kw):
            tl = os.path.join(tmp, "tiny-" + tag)
            trained_like_weights(prefix + ".wtw", tl + ".wtw", **kw)
            e4 = pkg.Engine(tl, vocab, True, device_id=local_rank)
            e4.set_option("stop_at_eot", 0)
            e4.set_option("kernel_timers", 4)
            eng_now.e = e4
            dt, _, n4, det4 = timed_leg(e4, d_mel.data_ptr(), B, 40, 12, args.depth, fence)
            leg = {"value": round(B * 40 * CLIP_SECONDS / dt, 1), "unit": "audio-sec/s", "steps": 40,
                   "ms_per_step": round(1e3 * dt / 40, 3), "f16_fallbacks": int(e4.get_option("f16_fallbacks")),
                   "f16_contractions": int(e4.get_option("f16_contractions")),
                   "min_slack_bits": round(e4.get_option("f16_min_slack_millibits") / 1000.0, 2),
                   "launches_per_step": {k: v["launches_per_step"] for k, v in det4.items()},
                   "all_clips_decoded": bool((n4 == 31).all()), "weights": what}
            e4.close()
            return leg

        leg = one("trained-like", "tools/wtw.py trained_like_weights(seed 4321): LayerNorm gains log-normal sigma 0.35 with 2 % of the "
                                  "channels 6..20 x, weight rows Student-t(4) entries with log-normal norms (sigma 0.5), residual "
                                  "channels 23 and 187 forty times the others, in every encoder layer")
        # far beyond published checkpoint statistics: row norms spread over e^+-4 (sigma 2) — where the check starts to act
        leg["extreme_row_spread"] = one("trained-like-x", "the same with row_sigma = 2.0 (row norms of every weight matrix spread "
                                                          "over a factor ~3000)", row_sigma=2.0)
        return leg

    # BASELINE.json configs[3] in the driver's line: whisper-base, batch 64, bf16 storage + bf16 MFMA
    def run_c3_leg():
        prefix3, vocab3 = ge._assets(tmp, "base", 0)
        e3 = pkg.Engine(prefix3, vocab3, True, device_id=local_rank)
        e3.set_option("bf16", 1)
        e3.set_option("stop_at_eot", 0)
        e3.set_option("kernel_timers", 4)
        B3 = 64
        eng_now.e = e3
        d_mel3 = e3.device_array(synthetic_mel(0, B3, e3.mel_shape))
        e3.device_synchronize()
        dt, _, n3, det3 = timed_leg(e3, d_mel3.data_ptr(), B3, 40, 6, 5, fence)
        dom3 = max(det3, key=lambda k: det3[k]["ms_per_step"]) if det3 else None
        tr3, tr3_src = traffic_from_profile(dom3, True, set(e3.kernel_stats())) if dom3 else (None, None)
        c3_leg = {"value": round(B3 * 40 * CLIP_SECONDS / dt, 1), "unit": "audio-sec/s", "steps": 40, "batches_in_flight": 5,
                  "ms_per_step": round(1e3 * dt / 40, 3), "dtype": "bf16 (weights, activations, KV caches; f32 accumulate)",
                  "config": {"workload": "whisper-base multilingual batch=64x30s synthetic mel U(-1,1.5), bf16 MFMA, random-init "
                                         "weights (BASELINE.json configs[3]); mel resident in HBM -> token ids on host"},
                  "all_clips_decoded": bool((n3 == 31).all()),
                  "roofline": ({"kernel": dom3, **{k: det3[dom3][k] for k in ("bound", "achieved", "peak", "unit", "frac", "avg_launch_us")},
                                "traffic": tr3, "traffic_source": tr3_src,
                                "note": "HIP events inside the pipelined region of this leg"} if dom3 else None),
                  "roofline_detail": det3}
        d_mel3.free()
        e3.close()
        return c3_leg

    iso = None
    if args.full and pipelined:
        # outside the timed region: two synchronous passes, so the per-kernel figures are also
        # reported without the encoder and the decoders sharing the chip
        iso_stats = {}
        eng.set_option("kernel_timers", 1)
        for _ in range(2):
            step()
            for name, v in eng.kernel_stats().items():
                acc = iso_stats.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
                for k in acc:
                    acc[k] += v[k]
        iso = iso_stats
    if rank == 0:
        total_clips = world * B * args.steps
        value = total_clips * CLIP_SECONDS / elapsed
        for k in stage:
            stage[k] = round(stage[k] / args.steps, 4)
        # dominant kernel = the class with the most device time inside the timed region
        detail = rooflines(kstats, max(1, sampled["steps"]))
        dom = max(detail, key=lambda k: detail[k]["ms_per_step"]) if detail else None
        roof = None
        if dom:
            d = detail[dom]
            # HBM-side bytes per launch of this kernel class come from separate rocprofv3 --pmc
            # passes (FETCH_SIZE, WRITE_SIZE) whose summary is committed under profiles/
            traffic, traffic_src = traffic_from_profile(dom, args.bf16, set(eng.kernel_stats()))
            roof = {"kernel": dom, "bound": d["bound"], "achieved": d["achieved"], "peak": d["peak"],
                    "unit": d["unit"], "frac": d["frac"], "traffic": traffic, "traffic_source": traffic_src,
                    **{k: d[k] for k in ("peak_is", "executed_16bit_tflops", "vs_fp32_mfma_peak") if k in d},
                    "algorithmic_flops_per_launch": int(kstats[dom]["flops"] / max(1, kstats[dom]["launches"])),
                    "avg_launch_us": d["avg_launch_us"]}
            if pipelined:
                # the pipelined encoder stream is CU-masked: what the launches reach of the CUs they may use
                cus = int(eng.get_option("pipelined_encoder_cus"))
                roof["pipelined_stream_cus"] = cus
                roof["frac_of_stream_cus"] = round(d["frac"] * 256.0 / cus, 4) if cus > 0 else None
        iso_det = rooflines(iso, 2) if iso else None
        # decoder phase against HBM: algorithmic bytes per step of this batch
        dm = eng.dims
        dstate, L, T, V = dm.n_text_state, dm.n_text_layer, dm.n_audio_ctx, dm.n_vocab
        esz = 2 if args.bf16 else 4                                    # bytes per stored element
        Hh = dm.n_text_head
        absorbed = bool(eng.get_option("cross_absorb_active"))
        paired = pipelined and absorbed and bool(eng.get_option("dec_pair")) and B <= int(os.environ.get("WT_PAIR_MAX_BATCH", "32")) and 2 * B <= 128
        group = max(1, min(int(eng.get_option("dec_group")), 128 // B)) if paired else 1
        if absorbed:
            # cross-attention against the encoder output itself: one [T][d] matrix of planes per clip and (layer, position)
            kv_bytes = L * T * dstate * 4 * B
            # q|k|v 3, out 1, absorbed query H, value (fp32, in the combine) 1, cross out 1, fc1 4, fc2 4 (x d^2, 4 B each)
            w_bytes = L * (14 + Hh) * dstate * dstate * 4
        else:
            kv_bytes = L * 2 * T * dstate * esz * B                  # cross KV read once per position
            w_bytes = L * 11 * dstate * dstate * esz + L * dstate * dstate * 4  # layer weights; the query projection is fp32 in both modes
        emb_bytes = V * dstate * esz                                   # tied embedding (logits GEMM)
        # the prompt's positions share one pass: 27 passes over the weights and the cache, 27 logits GEMMs; a decoder
        # chain that takes two batches together (dec_pair) reads the weights once for both
        rows = group * B                                               # 64 rows per pass: the 4 prompt positions go two and two; more: one by one
        n_pass = 27 if rows <= 32 else 28 if rows <= 64 else 30
        dec_bytes = n_pass * kv_bytes + n_pass * w_bytes // group + 27 * emb_bytes // group
        # decoder_ms is the chain's duration; a shared chain serves `group` steps
        dec_ms_per_step = stage["decoder_ms"] / group
        dec_ach = dec_bytes / (dec_ms_per_step * 1e-3) / 1e9 if dec_ms_per_step > 0 else 0.0
        out = {
            "metric": f"audio-sec/s (RTF) whisper-{args.arch} 30s clips batch={B} at 1/2/4/8 MI355X",
            "value": round(value, 1),
            "unit": "audio-sec/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16 (weights, activations, KV caches; f32 accumulate and residual stream)" if args.bf16 else
                     "f32 (operands as two fp16 planes, f16 MFMA, f32 accumulate)" if eng.get_option("gemm_variant") < 0 else "f32",
            "data": "synthetic",
            "config": {"workload": (f"whisper-{args.arch} multilingual batch={B}x30s synthetic mel U(-1,1.5), bf16 MFMA, random-init "
                                    "weights (BASELINE.json configs[3]); mel resident in HBM -> token ids on host") if args.bf16 else
                                   (f"whisper-{args.arch} batch={B}x30s synthetic mel U(-1,1.5), fp32, random-init "
                                    "weights (BASELINE.json configs[1]); mel resident in HBM -> token ids on host"),
                       "clips_per_gpu": B, "global_batch": world * B, "decoder_positions": 30,
                       "argmax_steps": 27, "parallelism": f"clip-parallel dp{world}, one RCCL all_gather of id records per {GATHER_EVERY} batches",
                       "pipelined": pipelined, "batches_in_flight": args.depth if pipelined else 1,
                       "decoder": f"{group} consecutive steps' batches share one decoder chain (dec_pair, dec_group)" if group > 1 else "one decoder chain per step",
                       "last_batches_announced": args.tail if pipelined else 0,
                       "priming_batches": 1,
                       "compute": "bf16 storage mode: weights, activations, the encoder output the decoder's cross-attention streams and the "
                                  "self-attention KV cache stored as bf16; every contraction one bf16 MFMA product with fp32 "
                                  "accumulation; residual streams, softmax statistics, LayerNorm, biases and the cross-attention value "
                                  "projection fp32" if args.bf16 else
                                  "every contraction (encoder GEMMs and attention, decoder GEMMs and logits): operands as 2 fp16 "
                                  "planes (22 significand bits: hi + lo, 4 bytes per element like fp32), 3 f16-MFMA products, "
                                  "fp32 accumulate (measured error at or below the fp32-MFMA kernel's, tests/test_gpu_kernels.py; "
                                  "bf16 x3 split and fp32 MFMA forms selectable); residual streams, softmax, LayerNorm fp32; decoder "
                                  "cross-attention on the encoder output's planes with the K / V projections absorbed (no KV cache)"},
        }
        # --full: what the headline does not need (event timers, isolated passes, stage events, legs, CPU baseline)
        full = {
            "roofline": ({**roof, "isolated": {k: iso_det[dom][k] for k in ("achieved", "frac", "avg_launch_us")},
                          "note": "achieved/avg_launch_us: HIP events inside the timed (pipelined) region, where decoder "
                                  "chains share the chip; isolated: the same launches in two synchronous passes after it — "
                                  "the figure a serialising profiler (rocprofv3 --kernel-trace, profiles/) reproduces.  The "
                                  "launch durations include the LayerNorms fused into the conv2 / out-projection / fc2 epilogues "
                                  "(9 per pass at 4 layers, 13 at 6: statistics, normalisation and the next operand's planes — "
                                  "work the flop count of the fraction does not credit)"}
                         if roof and iso_det and dom in iso_det else roof),
            "roofline_detail": detail,
            "roofline_isolated": iso_det,
            "decoder_roofline": {"bound": "hbm", "achieved": round(dec_ach, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                                 "frac": round(dec_ach / PEAK_HBM_GBPS, 4),
                                 "algorithmic_bytes_per_step": int(dec_bytes),
                                 "form": ("absorbed cross-attention (encoder output planes, K / V projections folded into the "
                                          "query / value sides)" if absorbed else "cross-KV cache") +
                                         (f", {group} batches per decoder chain" if group > 1 else ""),
                                 "chain_ms": round(stage["decoder_ms"], 3)},
            # what the headline assumes about the weights: every contraction whose weight-derived bound stays within 2^12
            # of its typical magnitude runs on two fp16 planes; the others (none here) on the full-range kernels
            "weights_assumption": {"weights": "random-init seed 0: Linear N(0, 1/fan_in), LayerNorm gain 1 / shift 0, embeddings "
                                              "N(0, 0.02^2) (there is no checkpoint in this environment)",
                                   "f16_contractions": int(eng.get_option("f16_contractions")),
                                   "f16_fallbacks": int(eng.get_option("f16_fallbacks")),
                                   "min_slack_bits": round(eng.get_option("f16_min_slack_millibits") / 1000.0, 2),
                                   "note": "slack = log2(4096 * typical / bound) of the tightest operand; a contraction with "
                                           "negative slack leaves the fp16-plane kernels (legs outlier_weights, "
                                           "trained_like_weights: count and cost)"},
            "encoder_fp32_mfma": fp32_leg,
            "outlier_weights": None,
            "trained_like_weights": None,
            "configs3_bf16_base": None,
            "with_frontend": with_frontend,
            "stage_ms_per_step": stage,
            "host_enqueue_ms_per_step": round(1e3 * host["submit_s"] / max(1, host["submits"]), 3) if pipelined else None,
        }
        if args.full:
            out.update(full)
        out["collectives"] = timed["collectives"]
        if args.report_maps:
            with open("/proc/self/maps") as f:
                out["hip_runtimes_mapped"] = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
        if args.emit_ids:
            out["gathered_records"] = timed["records"]
            out["ids_crc"] = timed["crc"]
            out["ids_digest"] = timed["digest"]
        if args.full and not args.no_cpu_baseline:
            info = eng.vocab_info()
            prompt = [info["sot"], 50259 + eng.get_option("language"), info["transcribe"], info["not"]]
            cb = cpu_baseline(prefix, mel_host, prompt, info["eot"])
            ids_c, n_c = cb.pop("ids"), cb.pop("n")
            k = ids_c.shape[0]
            cb["ids_match_gpu"] = bool(np.array_equal(ids_c[:, :31], ids[:k, :31]) and np.array_equal(n_c, n[:k]))
            out["cpu_baseline"] = cb
        if legs_ok:
            eng.close()
            out["outlier_weights"] = run_outlier_leg()
            out["trained_like_weights"] = run_trained_like_leg()
            out["configs3_bf16_base"] = run_c3_leg()
        print(json.dumps(out))
    eng.close()
    shutil.rmtree(tmp, ignore_errors=True)
    if world > 1 or FORCE_COLLECTIVES:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
