"""GPU (-m gpu): truncated sampling (options top_k / top_p).  (a) One step through
wt_dbg_sample_select_cut against nucleus_ref.step: the token is the reference's Gumbel argmax over N wherever the two best
keys differ by more than sample_ref's bar (at most one row in 64 under it, as test_gpu_sample_kernel.py allows) and a
member of N always.  (b) Through the engine on the EOT-rich micro model of scores_model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucleus_ref as nr  # noqa: E402
import scores_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu
SB, N0 = 2, len(sm.PLAIN_PROMPT)


@pytest.fixture(scope="module")
def plain(pkg, assets, tmp_path_factory):
    """(a debug engine on the micro model, the EOT-rich model's path, the vocabulary, four clips)"""
    prefix, vocab = assets("micro")
    path = str(tmp_path_factory.mktemp("nucleus") / "micro-plain")
    sm.write_plain_model(prefix + ".wtw", path + ".wtw")
    e = pkg.Engine(prefix, vocab, True)
    yield e, path, vocab, np.ascontiguousarray(sm.plain_mels()[:4])
    e.close()


def run_step(eng, z, gens, temps, group, top_k, top_p, ts, eot, beg, seed=3, attempt=1, clip_base=2):
    B, clips = z.shape[0], -(-z.shape[0] // group)
    ids = np.ones((B, SB + len(gens) + 1), np.int64)
    ids[:, SB:SB + len(gens)] = gens
    tok, _, _, _, cut = eng.dbg_sample_select_cut(z, ids, SB + len(gens), SB, temps, group, top_k, top_p, seed, attempt, clip_base,
                                                  0, -1, ts, eot, beg)
    under, infos = 0, []
    for r in range(B):
        want, info = nr.step(z[r], list(gens), temps[r % clips], top_k, top_p, seed, SB + len(gens) - 1, clip_base + r % clips,
                             attempt + (r // clips << 16), eot, beg, 50, ts)
        infos.append(info)
        assert info["fallback"] or int(tok[r]) in info["N"], (r, int(tok[r]))
        if info["fallback"] or info["gap"] > info["bar"]:
            assert int(tok[r]) == want, (r, int(tok[r]), want, info["gap"], info["bar"])
        else:
            under += 1
    assert under * 64 <= B, (under, B)
    return tok, cut, infos


@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("ts", [False, True])
@pytest.mark.parametrize("V", [4097, 51865])
def test_step_equals_the_reference(plain, V, ts, group):
    beg = V - 1501 if V > 8192 else V - 101
    eot = beg - 107 if V > 8192 else beg - 7
    z = (np.random.default_rng(V + 2 * ts + group).standard_normal((6, V)) * 3.0).astype(np.float32)  # flat rows: an open draw
    temps = np.array([0.6, 1.0, 0.8, 0.7, 0.9, 0.5], np.float32)[:-(-6 // group)]
    for top_k, top_p in ((5, 1.0), (50, 1.0), (0, 0.6), (40, 0.8)):
        _, cut, _ = run_step(plain[0], z, [beg + 3, 17] if ts else [], temps, group, top_k, top_p, ts, eot, beg)
        assert not top_k or (cut["kept"] <= top_k).all()


def test_rule_5_picks_timestamps_while_only_text_is_kept(plain):
    """The timestamps together outweigh the best text logit, each lies below it: top_k = 1 keeps one text id, rule 5
    leaves the timestamps, and the token is the largest timestamp logit."""
    V, beg, eot = 4097, 3996, 3989
    z = np.full((3, V), -20.0, np.float32)
    z[:, 100], z[:, beg + 4:], z[:, beg + 50] = 2.0, 1.0, 1.5
    tok, cut, infos = run_step(plain[0], z, [beg + 3, 17], np.array([0.6, 1.0, 0.8], np.float32), 1, 1, 1.0, True, eot, beg)
    assert all(i["fallback"] and i["mass"] for i in infos) and (tok == beg + 50).all() and (cut["kept"] == 1).all()


def decode(pkg, plain, positions=64, **options):
    e = pkg.Engine(plain[1], plain[2], True)
    for k, v in dict(options, max_positions=positions).items():
        e.set_option(k, v)
    ids, n = e.encdec_tokens_full(plain[3])
    e.close()
    return ids.tobytes() + n.tobytes(), ids, n


def test_engine_top_k_1_defaults_and_seed(pkg, plain):
    greedy = decode(pkg, plain)[0]
    for best_of in (1, 3):  # one kept id: the draw is the greedy step, on the full-length chain and the best-of chain
        assert decode(pkg, plain, temperature=1000, top_k=1, seed=5, best_of=best_of)[0] == greedy
    assert decode(pkg, plain, temperature=800, seed=9)[0] == decode(pkg, plain, temperature=800, seed=9, top_k=0, top_p=1000)[0]
    assert decode(pkg, plain, temperature=800, seed=9, top_p=900)[0] == decode(pkg, plain, temperature=800, seed=9, top_p=900)[0]


def test_every_id_of_a_top_k_5_run_is_among_the_five_largest(pkg, plain):
    """The steps' logits come from the teacher-forced debug pass over the sampled ids (a logit counts as larger only
    beyond 4e-4, twice the bound the two passes' fp32 logits agree within)."""
    _, ids, n = decode(pkg, plain, 32, temperature=1000, top_k=5, seed=4)
    assert decode(pkg, plain, 32)[0] != ids.tobytes() + n.tobytes()  # T = 1 over five ids leaves the greedy path
    e = pkg.Engine(plain[1], plain[2], True)
    e.set_forced_ids(np.ascontiguousarray(ids[:, :32]))
    logits = e.encdec_debug_batch(plain[3], want_enc_out=False)[3]
    e.close()
    for b in range(ids.shape[0]):
        for s in range(min(int(n[b]), 28) - N0):
            assert (logits[b, s] > logits[b, s, ids[b, N0 + s]] + 4e-4).sum() < 5, (b, s)


def test_values_out_of_range_are_refused(pkg, plain):
    e = pkg.Engine(plain[1], plain[2], True)
    for key, bad in (("top_k", -1), ("top_k", e.dims.n_vocab + 1), ("top_p", 0), ("top_p", 1001)):
        with pytest.raises(pkg.WtError) as err:
            e.set_option(key, bad)
        assert str(err.value).split(":")[0] == "WT_ERR_INVALID_ARG"
    assert e.get_option("top_k") == 0 and e.get_option("top_p") == 1000
    for k, v in (("top_k", e.dims.n_vocab), ("top_p", 1), ("max_positions", 32), ("temperature", 700)):
        e.set_option(k, v)
    assert (e.encdec_tokens_full(plain[3])[1] > N0).all()  # the engine stays usable
    e.close()
