"""Pins, on the CPU oracle, the inputs that tests/test_gpu_full_decode.py relies on (option max_positions, DESIGN.md
section 13), so that those tests cannot pass vacuously: the EOT-rich model of tests/full_model.py must finish clips
before position 32, between 33 and 159, and never; and the clips compared id by id must have no step whose top-two
logit margin is inside the decisive-margin bar.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import full_model as fm  # noqa: E402

P = fm.N_TEXT_CTX


@pytest.fixture(scope="module")
def rich_rows(orc, assets, tmp_path_factory):
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("full") / "micro-full-rich.wtw")
    fm.write_eot_rich(prefix + ".wtw", p)
    model = orc.Model(p)
    assert model.dims["n_text_ctx"] == P
    rows = fm.oracle_rows(model, fm.mels(fm.RICH_CLIPS, (80, 200), fm.RICH_SEED), fm.RICH_PROMPT, P, fm.EOT)
    model.close()
    return rows


def test_eot_rich_clips_finish_at_varied_positions(rich_rows):
    fin = [fm.finish_index(ids) for ids, _ in rich_rows]
    print("finishing index per clip:", fin)
    early = [b for b, f in enumerate(fin) if f is not None and f < 32]
    mid = [b for b, f in enumerate(fin) if f is not None and 33 <= f <= 159]
    capped = [b for b, f in enumerate(fin) if f is None]
    assert len(early) >= 2 and len(mid) >= 2 and len(capped) >= 1, fin
    for b in capped:  # positions 0 .. P - 1 fed: P + 1 ids
        assert len(rich_rows[b][0]) == P + 1
    for b, f in enumerate(fin):
        if f is not None:
            assert fm.EOT not in rich_rows[b][0][:f]


def test_eot_rich_margins_are_decisive(rich_rows):
    low = [float(m.min()) for _, m in rich_rows]
    print("smallest top-two margin per clip:", ["%.2e" % v for v in low])
    assert min(low) > 10 * fm.MARGIN, low


def test_dense_clips_and_their_margins(orc, assets, tmp_path_factory):
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("full") / "micro-full-dense.wtw")
    fm.write_dense(prefix + ".wtw", p)
    model = orc.Model(p)
    rows = fm.oracle_rows(model, fm.dense_mels((80, 200)), fm.DENSE_PROMPT, P, 50257)
    model.close()
    low = [float(m.min()) for _, m in rows]
    print("smallest top-two margin per dense clip:", ["%.2e" % v for v in low])
    for (ids, m), v in zip(rows, low):
        assert len(ids) == P + 1 and len(m) == P - len(fm.DENSE_PROMPT) + 1  # the micro vocabulary has no EOT
    # the GPU test may set ONE clip in six aside at an indecisive step; the chosen clips need none
    assert len(rows) == 6 and all(v >= fm.MARGIN for v in low), low


def test_positional_rows_are_extended_with_the_same_std(assets, tmp_path_factory):
    sys.path.insert(0, os.path.join(fm.ROOT, "tools"))
    from wtw import read_wtw
    prefix, _ = assets("micro")
    p = str(tmp_path_factory.mktemp("full") / "dense.wtw")
    fm.write_dense(prefix + ".wtw", p)
    d0, t0 = read_wtw(prefix + ".wtw")
    d1, t1 = read_wtw(p)
    assert d0["n_text_ctx"] == 64 and d1["n_text_ctx"] == P
    a, b = t0["decoder.positional_embedding"], t1["decoder.positional_embedding"]
    assert b.shape == (P, a.shape[1]) and np.array_equal(b[:64], a)
    assert abs(b[64:].std() / a.std() - 1.0) < 0.05
    for k in t0:
        if k != "decoder.positional_embedding":
            assert np.array_equal(t0[k], t1[k]), k
