"""The definitions of tests/sample_ref.py (options temperature, temperature_fallback): Philox
known answers, the uniform and the Gumbel term, T = 0 against ts_ref and the plain argmax, the distribution of the
sampler, the fall-back rule — and the pins of the fixtures of tests/sample_model.py on the CPU oracle, so that
tests/test_gpu_sampling.py cannot pass vacuously.  CPU only."""
import itertools
import math
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sample_model as smp  # noqa: E402
import sample_ref as sr  # noqa: E402
import scores_model as sm  # noqa: E402
import scores_ref  # noqa: E402
import ts_ref  # noqa: E402

# a small vocabulary: text 0..5, eot 6, specials 7..9, timestamps 10..19 (as tests/test_ts_reference.py)
V, EOT, BEG = 20, 6, 10


def hexes(c, k):
    return " ".join("%08x" % int(x) for x in sr.philox4x32_10(c, k))


def test_philox_known_answers():
    assert hexes((0, 0, 0, 0), (0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexes((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexes((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # the word of id i is word i & 3 of the call with counter (i >> 2, pos, clip, attempt), the key the seed's halves
    seed = (0x299F31D0 << 32) | 0xA4093822
    w = sr.words(11, 0x85A308D3, 0x13198A2E, 0x03707344, seed)
    for i in range(11):
        want = sr.philox4x32_10((i >> 2, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))[i & 3]
        assert int(w[i]) == int(want)


def test_uniform_is_exact_in_fp32_and_the_gumbel_range():
    x = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF], np.uint32)
    x = np.concatenate([x, np.random.default_rng(0).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)])
    u = sr.uniform_of(x)
    assert u.dtype == np.float32
    exact = ((x >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert np.array_equal(u.astype(np.float64), exact)  # no rounding anywhere
    assert u.min() == np.float32(2.0 ** -24) and u.max() == np.float32(1.0 - 2.0 ** -24) and 0.0 < u.min() and u.max() < 1.0
    g = sr.gumbel_of(u)
    assert g.min() == pytest.approx(-math.log(24 * math.log(2.0)), abs=1e-12) and -2.82 < g.min()
    assert g.max() == pytest.approx(-math.log(-math.log1p(-2.0 ** -24)), abs=1e-9) and g.max() < 16.64
    assert sr.inv_t_of(0.0) == 0.0 and sr.inv_t_of(0.2) == np.float32(1.0) / np.float32(0.2)
    assert sr.temperature_of_milli(200) == np.float32(200.0) / np.float32(1000.0)


def test_zero_temperature_is_the_greedy_step():
    rng = np.random.default_rng(1)
    for g in ([], [BEG + 1], [BEG + 1, 3], [BEG + 1, 3, BEG + 4], [BEG + 1, 3, BEG + 4, BEG + 4], [BEG + 9, 2]):
        for _ in range(20):
            z = np.round(rng.standard_normal(V) * 2, 1).astype(np.float32)  # ties: the larger id
            z[BEG:] += np.float32(rng.choice([-2.0, 0.0, 3.0]))
            tok, info = sr.step(z, g, 0.0, 5, 3, 1, 2, EOT, BEG, 3, True, check=True)
            want, ref = ts_ref.step(z, g, EOT, BEG, 3)
            assert tok == want and info["L"] == ref["L"] and info["M"] == ref["M"] and info["gap"] == ref["gap_top"]
            assert info["lp"] == scores_ref.token_logprob(z, tok, g, EOT, BEG, 3, True)[0]
            tok, info = sr.step(z, g, 0.0)
            assert tok == ts_ref._argmax_last(z, np.ones(V, bool)) and info["lp"] == scores_ref.token_logprob(z, tok)[0]


def test_a_step_is_the_keyed_argmax_over_the_allowed_set():
    rng = np.random.default_rng(2)
    z = rng.standard_normal(V).astype(np.float32)
    z[BEG:] += 1.0
    for g, T in itertools.product(([], [BEG + 1, 3], [BEG + 1, 3, BEG + 4]), (0.2, 1.0)):
        tok, info = sr.step(z, g, T, 9, 4, 2, 1, EOT, BEG, 50, True, check=True)
        mask, _ = sr.allowed_mask(z, g, EOT, BEG, 50, True)
        u = sr.uniform_of(sr.words(V, 4, 2, 1, 9))
        k = z.astype(np.float64) * float(sr.inv_t_of(T)) - np.log(-np.log(u.astype(np.float64)))
        k[~mask] = -np.inf
        assert tok == int(np.argmax(k)) and info["key"] == k[tok]
        rest = np.sort(k)[-2]
        assert info["gap"] == pytest.approx(k[tok] - rest) and info["bar"] > 0
        assert info["lp"] == scores_ref.token_logprob(z, tok, g, EOT, BEG, 50, True)[0]  # from the untempered logits
    # other counter words, other draws; the same words, the same draw
    a = [sr.step(z, [], 1.0, s, p, c, t)[0] for s, p, c, t in itertools.product((0, 1), (0, 1), (0, 1), (0, 1))]
    assert len(set(a)) > 4
    assert sr.step(z, [], 1.0, 1, 2, 3, 4)[0] == sr.step(z, [], 1.0, 1, 2, 3, 4)[0]
    # one allowed id: no second key
    one = np.full(V, -np.inf, np.float32)
    assert sr.step(z, [BEG + 9, 3, BEG + 9], 1.0, eot=EOT, beg=BEG, timestamps=True)[1]["gap"] > 0
    tok, info = sr.step(one, [], 1.0)
    assert tok == V - 1 and info["gap"] == 0.0 and info["lp"] == -math.inf  # all -inf: equal keys, the larger id


# 4096 draws (64 clips x 64 positions) from a row with eight dominant ids against its softmax; the statistic is
# chi-square with 7 degrees of freedom (99.9 % quantile 24.3) and, the generator being fixed, a constant
CHI2 = {500: 3.405, 1000: 6.704}


@pytest.mark.parametrize("milli", [500, 1000])
def test_the_sampler_draws_from_the_softmax(milli):
    Vb, top = 4101, [7, 600, 1023, 1024, 2500, 4095, 4096, 4100]
    z = np.full(Vb, -40.0, np.float32)
    z[top] = np.arange(8, dtype=np.float32) * np.float32(0.25)
    T = sr.temperature_of_milli(milli)
    p = np.exp(z[top].astype(np.float64) * float(sr.inv_t_of(T)))
    p /= p.sum()  # (the other ids hold exp(-40 / T) of the mass: none of 4096 draws)
    counts = np.zeros(8)
    for clip in range(64):
        for pos in range(64):
            tok, _ = sr.step(z, [], T, 2024, pos, clip, 1)
            counts[top.index(tok)] += 1
    chi2 = float(((counts - 4096 * p) ** 2 / (4096 * p)).sum())
    print("T = %.1f: counts %s, chi-square %.3f" % (float(T), counts.astype(int).tolist(), chi2))
    assert (4096 * p).min() > 40 and chi2 < 24.3
    assert chi2 == pytest.approx(CHI2[milli], abs=2e-3)


def test_fallback_rule_table():
    """Every combination of the three thresholds, on, off and on either side."""
    for cr, lp, ns in itertools.product((None, 2.4), (None, -1.0), (None, 0.6)):
        for ratio, avg, nsp in itertools.product((2.0, 2.4, 3.0), (-1.5, -1.0, -0.5), (0.3, 0.6, 0.9)):
            need = (cr is not None and ratio > cr) or (lp is not None and avg < lp)
            if ns is not None and lp is not None and nsp > ns and avg < lp:
                need = False
            assert sr.needs_fallback(ratio, avg, nsp, cr, lp, ns) == need, (cr, lp, ns, ratio, avg, nsp)
    assert sr.needs_fallback(3.0, -0.5, 0.1) and sr.needs_fallback(1.0, -1.5, 0.1) and not sr.needs_fallback(2.4, -1.0, 0.6)
    assert not sr.needs_fallback(3.0, -1.5, 0.9)   # silence: kept whatever its ratio
    assert sr.needs_fallback(3.0, -0.5, 0.9)       # ... but only below the log-probability threshold
    assert sr.schedule(0) == [0, 200, 400, 600, 800, 1000] and sr.schedule(200, 500) == [200, 700]
    assert sr.schedule(300, fallback=False) == [300] and sr.schedule(1000) == [1000]
    assert sr.compression_ratio(b"") == 0.0
    text = b"abc" * 40
    assert sr.compression_ratio(text) == len(text) / len(zlib.compress(text)) > 2.4


def test_fallback_loop_keeps_the_first_accepted_or_the_last():
    def rows(avgs):
        return lambda attempt, T: {"ids": [1, 2, 3 + attempt], "avg": avgs[attempt], "no_speech_prob": 0.1, "T": float(T)}
    temps = sr.schedule(0, 500)
    r = sr.decode_with_fallback(rows([-0.1, -9, -9]), lambda ids: b"x", temps)
    assert (r["attempts"], r["temperature_milli"], r["needs_fallback"], r["ids"]) == (1, 0, False, [1, 2, 3])
    r = sr.decode_with_fallback(rows([-2, -0.1, -9]), lambda ids: b"x", temps)
    assert (r["attempts"], r["temperature_milli"], r["needs_fallback"], r["T"]) == (2, 500, False, 0.5)
    r = sr.decode_with_fallback(rows([-2, -2, -2]), lambda ids: b"x", temps)
    assert (r["attempts"], r["temperature_milli"], r["needs_fallback"], r["ids"]) == (3, 1000, True, [1, 2, 5])
    r = sr.decode_with_fallback(rows([-0.1, -0.1, -0.1]), lambda ids: b"ab" * 100, temps)
    assert r["attempts"] == 3 and r["needs_fallback"] and r["compression_ratio"] == 200 / len(zlib.compress(b"ab" * 100))
    r = sr.decode_with_fallback(rows([-0.1]), lambda ids: b"ab" * 100, temps, compression_ratio_threshold=None)
    assert r["attempts"] == 1 and not r["needs_fallback"]


# ------------------------------------------------------------ the fixtures ---

# what the reference gives (chosen and first computed on the CPU): generated ids per clip at seed
# sample_model.SEED over P_LONG / P_PLAIN positions
TS_N = {200: [94, 14, 47, 71, 27, 11, 72, 82, 63, 82], 1000: [78, 94, 54, 94, 9, 23, 94, 41, 86, 94]}
PLAIN_N = {200: [20, 93, 71, 84, 16, 13, 26, 77, 39, 93, 46, 93], 1000: [19, 88, 63, 66, 16, 93, 22, 55, 34, 93, 31, 93]}
# the fall-back fixture: (attempts, final temperature in thousandths, needs_fallback, compression ratio) per clip
FB_PINS = [(3, 1000, 1, 2.5238), (3, 1000, 1, 5.4762), (2, 500, 0, 2.5294), (2, 500, 0, 7.1176), (1, 0, 0, 6.1333),
           (3, 1000, 1, 6.9333), (3, 1000, 1, 5.2381), (1, 0, 0, 2.4), (1, 0, 0, 2.2353), (3, 1000, 1, 4.3125)]


@pytest.fixture(scope="module")
def ref(orc, pkg, assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    d = tmp_path_factory.mktemp("sampling")
    paths = {"ts": str(d / "micro-scores-ts"), "plain": str(d / "micro-scores-plain")}
    sm.write_ts_model(prefix + ".wtw", paths["ts"] + ".wtw")
    sm.write_plain_model(prefix + ".wtw", paths["plain"] + ".wtw")
    r = smp.Reference(orc, paths, {"ts": sm.ts_mels(), "plain": sm.plain_mels()})
    r.vocab = pkg.Vocab(vocab)
    yield r
    r.close()


def test_zero_temperature_equals_the_greedy_references_on_the_fixtures(ref):
    for mode, P, ts in (("ts", smp.P_SHORT, True), ("plain", sm.P_PLAIN, False)):
        model = ref.orc.Model(ref.paths[mode] + ".wtw")
        want = sm.reference(model, ref.mels[mode][:3], P, ts)
        model.close()
        for b in range(3):
            got = ref.row(mode, b, b, 0, 99, P, check=True)
            assert got["ids"] == want[b]["ids"] and got["lps"] == want[b]["lps"] and got["avg"] == want[b]["avg"]
            assert got["no_speech_prob"] == want[b]["no_speech_prob"]


@pytest.mark.parametrize("mode", ["ts", "plain"])
def test_fixed_temperature_fixture_pins(ref, mode):
    P = sm.P_LONG if mode == "ts" else sm.P_PLAIN
    n_clips = ref.mels[mode].shape[0]
    pins = TS_N if mode == "ts" else PLAIN_N
    for milli in smp.TEMPS:
        rows = [ref.row(mode, b, b, milli, smp.SEED, P) for b in range(n_clips)]
        n = [r["n"] for r in rows]
        decisive = [smp.compared_steps(r, milli) == r["n"] for r in rows]
        print(mode, milli, "n", n, "decisive", decisive, "smallest gap %.3e" % min(i["gap"] for r in rows for i in r["infos"]))
        assert n == pins[milli]
        assert sum(decisive) >= (8 if mode == "ts" else 10)
        greedy = [ref.row(mode, b, b, 0, smp.SEED, P)["ids"] for b in range(3)]
        if milli == 1000:
            assert any(rows[b]["ids"] != greedy[b] for b in range(3))  # the sampler is not the argmax in disguise
        for r in rows:
            assert np.isfinite(r["lps"]).all() and max(r["lps"]) <= 0.0
        # another seed, another decode
        other = ref.row(mode, 0, 0, milli, smp.OTHER_SEED, P)
        assert milli == 200 or other["ids"] != rows[0]["ids"]
    short = [smp.cut(ref.row(mode, b, b, 200, smp.SEED, P), smp.P_SHORT, 3 if mode == "ts" else 4) for b in range(2)]
    for b in range(2):
        direct = sr.decode(ref._fn(mode, b), sm.TS_PROMPT if mode == "ts" else sm.PLAIN_PROMPT, smp.P_SHORT, sm.EOT, sm.NOSP,
                           sr.temperature_of_milli(200), smp.SEED, b, 0, sm.BEG, mode == "ts")
        assert direct["ids"] == short[b]["ids"] and direct["lps"] == short[b]["lps"]  # the cut is the shorter decode


def test_fallback_fixture_pins(ref):
    rows = ref.fallback(smp.text_of_vocab(ref.vocab))
    got = [(r["attempts"], r["temperature_milli"], int(r["needs_fallback"]), round(r["compression_ratio"], 4)) for r in rows]
    print(got)
    assert got == FB_PINS
    last = smp.FB_TEMPS[-1]
    assert smp.FB_TEMPS == [0, 500, 1000]
    kinds = {"at_zero": [b for b, g in enumerate(got) if g[0] == 1],
             "intermediate": [b for b, g in enumerate(got) if g[1] not in (0, last)],
             "exhausted": [b for b, g in enumerate(got) if g[1] == last and g[2] == 1]}
    assert all(kinds.values()), kinds
    lp_thr, ns_thr, cr_thr = (smp.FB[k] / 1000.0 for k in ("logprob_threshold", "no_speech_threshold", "compression_ratio_threshold"))
    silent = [b for b, r in enumerate(rows) if r["no_speech_prob"] > ns_thr and r["avg"] < lp_thr]
    assert silent and all(not rows[b]["needs_fallback"] for b in silent)  # kept by the silence exemption
    assert any(rows[b]["compression_ratio"] > cr_thr for b in silent)     # ... although the ratio alone asks for more
    # every decision of every attempt lies clear of its thresholds: the engine's fp32 scores cannot decide otherwise
    text_of = smp.text_of_vocab(ref.vocab)
    for b, r in enumerate(rows):
        for attempt in range(r["attempts"]):
            a = ref.row("ts", b, b, smp.FB_TEMPS[attempt], smp.FB["seed"], smp.P_SHORT, attempt)
            assert abs(a["avg"] - lp_thr) > 5e-3 and abs(a["no_speech_prob"] - ns_thr) > 0.02
            assert abs(sr.compression_ratio(text_of(a["ids"], 3)) - cr_thr) > 0.05
            assert smp.compared_steps(a, smp.FB_TEMPS[attempt]) == a["n"]  # and every step of it is decisive
