"""The scenario of tests/longform_batch_model.py pinned on the CPU oracle (oracle front end + decoder + tests/longform_ref.py),
so that tests/test_gpu_longform_batch.py cannot pass vacuously: every file's reference run is decisive, and the rounds the
batched loop forms exercise what per-clip contexts are for.  CPU only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import longform_batch_model as bm  # noqa: E402
import longform_model as lm  # noqa: E402
import longform_ref as lr  # noqa: E402


@pytest.fixture(scope="module")
def runs(pkg, orc, assets, tmp_path_factory):
    """The reference run of every file alone, under the scenario's options."""
    prefix, vocab_path = assets("micro")
    p = str(tmp_path_factory.mktemp("longform_batch") / "micro-longform.wtw")
    lm.write_model(prefix + ".wtw", p)
    vocab = pkg.Vocab(vocab_path, True)
    filters, fe = vocab.filters(), orc.frontend()
    model = orc.Model(p)
    assert model.dims["n_text_ctx"] == lm.N_TEXT_CTX and 2 * model.dims["n_audio_ctx"] * 160 == bm.WIN
    try:
        return [bm.reference(model, lambda f, x, seek: fe.logmel(lm.window(x, seek), filters, 8), f)
                for f in range(len(bm.FILES))]
    finally:
        model.close()
        vocab.close()


def test_the_files(runs):
    assert len(bm.FILES) == 4 and bm.VARIANTS[0] == bm.SCENARIO == (True, (), True)
    for f, ws in enumerate(runs):
        print(f, [(r["seek"], r["advance"], r["n_context"], r["n_prompt"], len(r["ids"]), int(r["skipped"]), len(r["kept"]),
                   "%.2f" % r["no_speech_prob"]) for r in ws])
    assert bm.pcm(0).tobytes() == lm.pcm().tobytes() and len(runs[0]) >= 6
    assert len(runs[1]) >= 4
    assert bm.pcm(2).size < bm.WIN and len(runs[2]) == 1
    # file 3: skip_silence blanks its first windows and its context stays empty, while file 0's has grown to the truncated one
    assert all(r["skipped"] and r["n_context"] == 0 for r in runs[3][:6]) and any(r["kept"] for r in runs[3])
    assert any(r["n_context"] == bm.KEEP for r in runs[0][:6])


def test_every_file_is_decisive_over_all_its_windows(runs):
    for f, ws in enumerate(runs):
        assert lr.smallest_margin(ws) > bm.MARGIN, f
        assert all(abs(r["no_speech_prob"] - lm.NO_SPEECH_THRESHOLD / 1000) > 0.05 for r in ws), f  # skip_silence decides on them alone


def test_the_scenario_exercises_what_the_feature_is_for(runs):
    rounds = bm.rounds(runs)
    lengths = [sorted({r["n_prompt"] for _, r in rd}) for rd in rounds]
    print("fed-prompt lengths in flight per round:", lengths)
    assert sum(1 for s in lengths if len(s) >= 3) >= 3
    assert any({0, bm.KEEP} <= {r["n_context"] for _, r in rd} for rd in rounds)
    assert any(len(rd) < len(bm.FILES) for rd in rounds[1:])  # a round after a file has ended
    # a clip stops at its own position cap — P + 1 ids, no EOT among the generated ones — while a clip behind a shorter
    # prompt is still generating: in slots, the latter's last id lies behind the former's
    def capped(r):
        return len(r["ids"]) == bm.P + 1 and lm.EOT not in r["ids"][r["n_prompt"]:-1]
    assert any(capped(a) and b["n_prompt"] < a["n_prompt"] and len(b["ids"]) - b["n_prompt"] > len(a["ids"]) - a["n_prompt"]
               for rd in rounds for _, a in rd for _, b in rd)
