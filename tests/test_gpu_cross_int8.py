"""GPU (-m gpu): option cross_int8 through the engine on the micro model: the option, the logits
against the float64 decoder with the same quantisers, and the decode chains with and without graphs."""
import numpy as np
import pytest

import cross_int8_ref as ref
import mode_schedule as ms
from wtw import read_wtw
from test_gpu_graph_isolation import world  # noqa: F401 (fixture: the schedule's model, fresh engines, references)

pytestmark = pytest.mark.gpu
CLIPS32 = tuple(i % len(ms.Data().mel) for i in range(32))   # synchronous greedy calls take the absorbed form from 32 clips on
KINDS = [ms.Kind("cross8/short", "short", "batch", CLIPS32, {}),   # (31-position calls return ids alone)
         ms.Kind("cross8/full40", "full40", "full", CLIPS32, dict(max_positions=40, scores=1)),
         ms.Kind("cross8/beam2", "wide", "full", ms.C2, dict(max_positions=40, full_beam=1, beam_size=2, scores=1))]


@pytest.fixture(scope="module")
def micro(pkg, assets):
    prefix, vocab = assets("micro")

    def make():
        e = pkg.Engine(prefix, vocab, True)
        e.set_option("stop_at_eot", 0)
        e.set_prompt([3, 5, 7, 11])   # the micro vocabulary has no special ids
        e.set_option("max_tokens", 9)  # a four-id prompt and 6 argmax steps
        return e
    mel = np.random.default_rng(41).uniform(-1.0, 1.5, size=(32, 80, 200)).astype(np.float32)
    return make, read_wtw(prefix + ".wtw"), mel


def test_option_and_accuracy(pkg, micro):
    """0 and 1 alone; back at 0, a 32-clip call gives an untouched engine's ids and logits bit for bit.  On, section 38's
    protocol: per row within D / 2 of the float64 decoder with this option's quantisers, D that row's distance between
    the quantised and the unquantised float64 decoders (a fake-quantised path is discontinuous)."""
    make, (dims, tensors), mel = micro
    plain, e = make(), make()
    try:
        ids0, _, enc, lg0 = plain.encdec_debug_batch(mel, steps_cap=6)
        with pytest.raises(pkg.WtError) as err:
            e.set_option("cross_int8", 2)
        assert err.value.code == 1 and e.get_option("cross_int8") == 0
        e.set_option("cross_int8", 1)
        assert e.get_option("cross_int8") == 1
        e.set_forced_ids(ids0)
        lg_on = e.encdec_debug_batch(mel, steps_cap=6)[3]
        e.set_forced_ids(None)
        e.set_option("cross_int8", 0)
        ids2, _, _, lg2 = e.encdec_debug_batch(mel, steps_cap=6)
    finally:
        plain.close()
        e.close()
    assert np.array_equal(ids2, ids0) and np.array_equal(lg2.view(np.uint32), lg0.view(np.uint32))
    for b in (0, 17, 31):
        q, u = (ref.decoder_logits(dims, tensors, list(ids0[b, :9]), enc[b], quantised)[3:] for quantised in (True, False))
        err, D = np.abs(lg_on[b] - q).max(axis=1), np.abs(q - u).max(axis=1)
        print(f"clip {b}: err / D per step {np.array2string(err / D, precision=3)}, D {np.array2string(D, precision=3)}")
        assert (np.abs(lg0[b] - u).max(axis=1) < 1e-4).all()   # the reference is this engine's decoder
        assert (err < D / 2).all(), (b, err, D)


@pytest.mark.parametrize("kind", KINDS, ids=[k.name for k in KINDS])
def test_chains_graphs_and_switching(world, kind):
    """31 positions, 40 in two segments, beam search over them: the eager engine with the option on differs from the one
    that never heard of it; an engine WITH graphs that switches it between calls matches them byte for byte, call by call."""
    off = world.expected(kind)
    eng = world.engine(False)
    try:
        eng.set_option("cross_int8", 1)
        on = world.run(eng, kind)
    finally:
        eng.close()
    assert not kind.options or ms.first_difference(on, off) is not None   # (the log-probabilities move)
    eng = world.engine(True)
    try:
        for v in (1, 0, 1, 0):
            eng.set_option("cross_int8", v)
            diff = ms.first_difference(world.run(eng, kind), on if v else off)
            assert diff is None, (v, diff)
    finally:
        eng.close()
    if kind.name != "cross8/full40":
        return
    # the decisive positions of clip 0 (top-two margin above twice the bar D / 2) are the quantised float64 decoder's argmax
    dims, tensors = read_wtw(world.prefix + ".wtw")
    eng = world.engine(False)
    try:
        ms.reset(eng)
        enc = eng.encdec_debug_batch(world.data.mel[[kind.clips[0]]], want_logits=False)[2][0]
    finally:
        eng.close()
    ids, n = ms.ids_of(on)
    row, n_prompt = [int(i) for i in ids[0, :n[0]]], len(ms.PROMPT)
    q = ref.decoder_logits(dims, tensors, row[:-1], enc, True)[n_prompt - 1:]
    u = ref.decoder_logits(dims, tensors, row[:-1], enc, False)[n_prompt - 1:]
    top2 = np.sort(q, axis=1)[:, -2:]
    decisive = top2[:, 1] - top2[:, 0] > np.abs(q - u).max(axis=1)
    assert decisive.sum() >= 3 and (q.argmax(axis=1)[decisive] == np.asarray(row[n_prompt:])[decisive]).all()
