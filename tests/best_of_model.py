"""Fixtures of the best-of tests (option best_of): the models and clips of tests/sample_model.py,
the cases and the seeds chosen on them on the CPU, and the reference — tests/best_of_ref.py over tests/sample_ref.py
over the CPU oracle.  tests/test_best_of_reference.py pins what they give.

A clip of a case is DECISIVE when every one of its samples is decisive over its whole path (sample_model.compared_steps)
and its best two averages differ by more than AVG_GAP.  Each token log-probability is within section 15's 1.1e-4 of the
reference, so each average is too, and two averages may move towards each other by twice that: 2.2e-4.  The seed of a
case is the first in 1 .. 32 for which every clip is decisive (choose_seed); where none is, the one that sets the fewest
clips aside, at most one in five, and SET_ASIDE names them."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import best_of_ref as bo  # noqa: E402
import sample_model as smp  # noqa: E402
import scores_model as sm  # noqa: E402

AVG_GAP = 2.2e-4
# name -> mode, samples, temperature (thousandths), clips, positions.  Clip b of a case is mel clip b % 10 under the
# Philox clip index b.
CASES = {
    "ts-5x5-hot": ("ts", 5, 1000, 5, smp.P_SHORT),
    "ts-2x5-cool": ("ts", 2, 200, 5, smp.P_SHORT),
    "plain-2x1-long": ("plain", 2, 1000, 1, sm.P_PLAIN),
    "ts-5x26-hot": ("ts", 5, 1000, 26, smp.P_SHORT),   # 25 clips fill a chain's 125 rows; the 26th runs a second chain
}
# chosen by choose_seed on the CPU oracle; pinned by tests/test_best_of_reference.py
SEEDS = {"ts-5x5-hot": 2, "ts-2x5-cool": 3, "plain-2x1-long": 1, "ts-5x26-hot": 11}
SET_ASIDE = {"ts-5x5-hot": (), "ts-2x5-cool": (1,), "plain-2x1-long": (), "ts-5x26-hot": ()}


def n_mel(ref, mode):
    return ref.mels[mode].shape[0]


def clip_samples(ref, mode, b, N, milli, seed, P, attempt=0, clip=None):
    """(picked, rows) of clip b: sample j is sample_ref.decode under the attempt word attempt + (j << 16)."""
    clip = b if clip is None else clip
    return bo.decode_samples(lambda w: ref.row(mode, b % n_mel(ref, mode), clip, milli, seed, P, w), N, attempt)


def decisive(rows, picked, milli):
    if any(smp.compared_steps(r, milli) != r["n"] for r in rows):
        return False
    avgs = sorted((r["sum"] / r["n"] for r in rows), reverse=True)
    return len(avgs) < 2 or avgs[0] - avgs[1] > AVG_GAP


def case_rows(ref, name, seed=None):
    """[(picked, rows, decisive)] per clip of a case."""
    mode, N, milli, clips, P = CASES[name]
    seed = SEEDS[name] if seed is None else seed
    out = []
    for b in range(clips):
        picked, rows = clip_samples(ref, mode, b, N, milli, seed, P)
        out.append((picked, rows, decisive(rows, picked, milli)))
    return out


def choose_seed(ref, name, seeds=range(1, 33)):
    """(seed, clips set aside): the first seed under which every clip is decisive, else the one with the fewest aside."""
    best = None
    for seed in seeds:
        aside = tuple(b for b, (_, _, ok) in enumerate(case_rows(ref, name, seed)) if not ok)
        ref.rows.clear()  # (a search keeps nothing)
        if not aside:
            return seed, aside
        if best is None or len(aside) < len(best[1]):
            best = (seed, aside)
    return best


def make_reference(orc, paths, mels=None):
    mels = {"ts": sm.ts_mels(), "plain": sm.plain_mels()} if mels is None else mels
    return smp.Reference(orc, paths, mels)


# The fall-back fixtures: sample_model's (timestamp model, schedule 0 / 0.5 / 1.0, its seed) with FB_N samples at the
# attempts above temperature 0.  "fallback": the attempt at 0 is the greedy decode, under sample_model's thresholds.
# "fallback_beam" (option fallback_beam): the attempt at 0 is beam_full_ref.beam_search with FB_K hypotheses, under
# FB_BEAM's thresholds, chosen on the CPU as section 19 chose its own: no decision of any attempt within 5e-3
# (avg_logprob), 0.02 (no_speech_prob) or 0.05 (ratio) of its threshold, clips kept from the beam and from best-of attempts.
FB_N = 3
FB_K = 4
BEAM_DELTA = 2e-4  # section 23: a search is decisive when its smallest decision gap is above it
# Clips 2, 3, 4, 7 and 8 are accepted from the beam; clip 0 (ratio 6.6 at 0 and at 0.5) is accepted at 1.0 from sample 0 of
# 3 (ratio 2.52, avg_logprob -0.277); clips 1, 5, 6 and 9 exhaust the schedule on their ratio.
FB_BEAM = dict(smp.FB, logprob_threshold=-300, compression_ratio_threshold=2600)


def beam_row(ref, b, K, P):
    """Clip b of the timestamp fixture by beam_full_ref.beam_search, in the form of sample_ref.decode's dict (n counts
    EOT; margin = the search's smallest decision gap)."""
    import beam_full_ref as bfr
    import scores_ref
    key = ("beam", b, K, P)
    if key not in ref.rows:
        fn = ref._fn("ts", b)  # (loads the model and the clip's encoder output)
        r = bfr.beam_search(bfr.level_logits_fn(ref.models["ts"], ref.enc[("ts", b)], sm.EOT), sm.TS_PROMPT, K, P, sm.EOT,
                            sm.BEG, True)
        nsp = scores_ref.no_speech_prob(fn(list(sm.TS_PROMPT[:1])), sm.NOSP)
        ref.rows[key] = {"ids": r["ids"], "lps": r["lps"], "sum": r["sum"], "n": r["n_gen"], "avg": r["sum"] / r["n_gen"],
                         "no_speech_prob": nsp, "infos": [], "margin": r["margin"], "temperature": 0.0}
    return ref.rows[key]


def fallback_rows(ref, text_of, clips=None, clip_base=0, N=FB_N, fb=smp.FB, P=smp.P_SHORT, beam=0):
    """sample_ref.decode_with_fallback per clip, an attempt above 0 being the kept one of N samples and the attempt at 0
    the greedy decode or, with beam = K > 1, the beam search; each result carries picked, samples (the kept attempt's
    rows) and tried (every attempt's (picked, rows))."""
    import sample_ref as sr
    clips = list(range(n_mel(ref, "ts"))) if clips is None else list(clips)
    temps = sr.schedule(fb["temperature"], fb["temperature_increment"])
    out = []
    for i, b in enumerate(clips):
        tried = []

        def decode_at(attempt, T, b=b, i=i, tried=tried):
            if temps[attempt] == 0:
                picked, rows = 0, [beam_row(ref, b, beam, P) if beam > 1 else ref.row("ts", b, clip_base + i, 0, fb["seed"], P, attempt)]
            else:
                picked, rows = clip_samples(ref, "ts", b, N, temps[attempt], fb["seed"], P, attempt, clip_base + i)
            tried.append((picked, rows))
            return dict(rows[picked], picked=picked, samples=rows)

        r = sr.decode_with_fallback(decode_at, lambda ids: text_of(ids, len(sm.TS_PROMPT)), temps,
                                    fb["compression_ratio_threshold"] / 1000.0, fb["logprob_threshold"] / 1000.0,
                                    fb["no_speech_threshold"] / 1000.0)
        out.append(dict(r, tried=tried))
    return out


# ---- the recorded reference (tests/golden/best_of_rows.npz): what the GPU tests compare with, so that they need no
# oracle run; tests/test_best_of_reference.py recomputes it from the oracle ----
GOLDEN = os.path.join(ROOT, "tests", "golden", "best_of_rows.npz")


def pack_rows(rows_per_clip, P, milli):
    """[[row per sample] per clip] -> arrays: ids int32 [clips][N][P + 1] (-1 behind the row), n_ids, lps float64
    [clips][N][P], compared (the generated ids the engine must reproduce) and no_speech_prob [clips]."""
    clips, N = len(rows_per_clip), max(len(r) for r in rows_per_clip)
    ids = np.full((clips, N, P + 1), -1, np.int32)
    n_ids = np.zeros((clips, N), np.int32)
    lps = np.zeros((clips, N, P), np.float64)
    comp = np.zeros((clips, N), np.int32)
    nosp = np.zeros(clips, np.float64)
    for c, rows in enumerate(rows_per_clip):
        nosp[c] = rows[0]["no_speech_prob"]
        for j, r in enumerate(rows):
            ids[c, j, : len(r["ids"])] = r["ids"]
            n_ids[c, j] = len(r["ids"])
            lps[c, j, : r["n"]] = r["lps"]
            comp[c, j] = smp.compared_steps(r, milli)
    return {"ids": ids, "n_ids": n_ids, "lps": lps, "compared": comp, "nosp": nosp}


def case_arrays(ref, name, seed=None):
    mode, N, milli, clips, P = CASES[name]
    got = case_rows(ref, name, seed)
    a = pack_rows([rows for _, rows, _ in got], P, milli)
    a["picked"] = np.array([p for p, _, _ in got], np.int32)
    a["decisive"] = np.array([ok for _, _, ok in got], bool)
    return a


def fallback_arrays(ref, text_of, beam=0):
    rows = fallback_rows(ref, text_of, fb=FB_BEAM if beam > 1 else smp.FB, beam=beam)
    a = pack_rows([[r] for r in rows], smp.P_SHORT, 1000)
    a["picked"] = np.array([r["picked"] for r in rows], np.int32)
    a["attempts"] = np.array([r["attempts"] for r in rows], np.int32)
    a["milli"] = np.array([r["temperature_milli"] for r in rows], np.int32)
    a["needs"] = np.array([r["needs_fallback"] for r in rows], np.int32)
    a["ratio"] = np.array([r["compression_ratio"] for r in rows], np.float64)
    G = bo.N_MAX
    a["all_sum"], a["all_count"] = np.zeros((len(rows), G)), np.zeros((len(rows), G), np.int32)
    a["same"] = np.zeros((len(rows), G), np.int32)  # samples whose ids are the kept one's: a tie among them is no decision
    a["margin"] = np.array([r.get("margin", np.inf) for r in rows])  # of a clip kept from the beam: the search's own
    for c, r in enumerate(rows):
        a["same"][c, : len(r["samples"])] = [x["ids"] == r["ids"] for x in r["samples"]]
        a["all_sum"][c, : len(r["samples"])] = [x["sum"] for x in r["samples"]]
        a["all_count"][c, : len(r["samples"])] = [x["n"] for x in r["samples"]]
    return a, rows


def fallback_margins(rows, text_of, fb=smp.FB):
    """The smallest distance of any attempt's decision from its threshold: (avg_logprob, no_speech_prob, compression
    ratio), whether every sample of every attempt is decisive, and the smallest gap between an attempt's kept average and
    the best average of a sample with other ids."""
    import sample_ref as sr
    temps = sr.schedule(fb["temperature"], fb["temperature_increment"])
    d_avg = d_nosp = d_ratio = gap = float("inf")
    ok = True
    for r in rows:
        for attempt, (picked, samples) in enumerate(r["tried"]):
            k = samples[picked]
            d_avg = min(d_avg, abs(k["avg"] - fb["logprob_threshold"] / 1000.0))
            d_nosp = min(d_nosp, abs(k["no_speech_prob"] - fb["no_speech_threshold"] / 1000.0))
            d_ratio = min(d_ratio, abs(sr.compression_ratio(text_of(k["ids"], len(sm.TS_PROMPT))) - fb["compression_ratio_threshold"] / 1000.0))
            ok = ok and all(x["margin"] > BEAM_DELTA if "margin" in x else smp.compared_steps(x, temps[attempt]) == x["n"]
                            for x in samples)
            rest = [x["avg"] for x in samples if x["ids"] != k["ids"]]  # (samples that drew the kept ids tie with it exactly)
            if rest:
                gap = min(gap, k["avg"] - max(rest))
    return d_avg, d_nosp, d_ratio, ok, gap


def load_golden():
    with np.load(GOLDEN) as z:
        out = {}
        for key in z.files:
            case, field = key.split("/")
            out.setdefault(case, {})[field] = z[key]
    return out


if __name__ == "__main__":
    # python tests/best_of_model.py <ts prefix> <plain prefix> <vocab> search [case ...]   the seed search
    # python tests/best_of_model.py <ts prefix> <plain prefix> <vocab> golden             writes GOLDEN
    import time

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    r = make_reference(ge.load_oracle(), {"ts": sys.argv[1], "plain": sys.argv[2]})
    if sys.argv[4] == "search":
        for name in sys.argv[5:] or CASES:
            t0 = time.time()
            seed, aside = choose_seed(r, name)
            rows = case_rows(r, name, seed)
            print(name, "seed", seed, "aside", aside, "picked", [p for p, _, _ in rows],
                  "n_ids", [[len(x["ids"]) for x in rs] for _, rs, _ in rows], "%.1f s" % (time.time() - t0), flush=True)
    else:
        text_of = smp.text_of_vocab(ge.load_package().Vocab(sys.argv[3]))
        out = {}
        for name in CASES:
            for k, v in case_arrays(r, name).items():
                out[name + "/" + k] = v
            print(name, "picked", out[name + "/picked"].tolist(), "decisive", out[name + "/decisive"].tolist(), flush=True)
        fa, rows = fallback_arrays(r, text_of)
        for k, v in fa.items():
            out["fallback/" + k] = v
        print("fallback", list(zip(fa["attempts"].tolist(), fa["milli"].tolist(), fa["needs"].tolist(), fa["picked"].tolist())),
              "margins", fallback_margins(rows, text_of))
        fa, rows = fallback_arrays(r, text_of, FB_K)
        for k, v in fa.items():
            out["fallback_beam/" + k] = v
        print("fallback_beam", list(zip(fa["attempts"].tolist(), fa["milli"].tolist(), fa["needs"].tolist(), fa["picked"].tolist())),
              "margins", fallback_margins(rows, text_of, FB_BEAM))
        np.savez_compressed(GOLDEN, **out)
    r.close()
