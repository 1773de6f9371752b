"""Replayed decoder graphs against a fresh engine, across modes.  Every decode entry point replays
its launch sequence from a captured hipGraph found under a hand-written key, and a captured graph freezes every kernel
argument; so every setting that changes a launch constant must be in the key, and every reallocation must destroy
exactly the graphs that hold the old address.  The feature tests check use_graphs 0 against 1 inside their own mode;
these run the modes of tests/mode_schedule.py against one another on ONE engine and compare every value.

The reference of a kind is its result on an engine created for it alone with use_graphs = 0, run once: no captured
graph and no earlier call.  It is compared byte for byte."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mode_schedule as ms  # noqa: E402

pytestmark = pytest.mark.gpu

WARM = ms.with_clips(ms.KINDS["short/default"], ms.C6)   # sizes the workspace once, so that no schedule grows it
STABLE = {"short": "short/default", "full40": "full40/ts_scores", "full96": "full96/fallback",
          "wide": "wide/fallback_beam", "seek": "seek/long"}


class World:
    def __init__(self, pkg, prefix, vocab):
        self.pkg, self.prefix, self.vocab, self.data = pkg, prefix, vocab, ms.Data()
        self._expected = {}

    def engine(self, graphs):
        eng = self.pkg.Engine(self.prefix, self.vocab, True)
        eng.set_option("use_graphs", int(graphs))
        return eng

    def run(self, eng, kind):
        return ms.run(self.pkg, eng, kind, self.data)

    def fresh(self, kind):
        eng = self.engine(False)
        try:
            return self.run(eng, kind)
        finally:
            eng.close()

    def expected(self, kind):
        if kind.name not in self._expected:
            self._expected[kind.name] = self.fresh(kind)
        return self._expected[kind.name]


@pytest.fixture(scope="module")
def world(pkg, assets, tmp_path_factory):
    prefix, vocab = assets("micro")
    p = str(tmp_path_factory.mktemp("graph-isolation") / "micro-schedule")
    ms.write_model(prefix + ".wtw", p + ".wtw")
    return World(pkg, p, vocab)


class Visits:
    """One engine's calls: every result against the kind's reference, and what graphs_cached may do at each."""

    def __init__(self, world, graphs=True, warm=True):
        self.w, self.graphs, self.eng = world, graphs, world.engine(graphs)
        self.history, self.slot, self.seen = [], 0, set()
        if warm:
            self.visit(WARM)

    def close(self):
        self.eng.close()

    def cached(self):
        return self.eng.get_option("graphs_cached")

    def visit(self, kind, replay=False):
        """Runs the kind and compares; replay: the visit must find every graph it needs (graphs_cached unchanged, but for
        31-position beam search in a pipeline slot that kind has not run in: one capture).  Returns the growth."""
        before, prev = self.cached(), self.history[-1].name if self.history else "nothing"
        got = self.w.run(self.eng, kind)
        self.history.append(kind)
        growth = self.cached() - before
        diff = ms.first_difference(got, self.w.expected(kind))
        if diff is not None:
            pytest.fail("%s (after %s, call %d, use_graphs = %d): field %s differs from the fresh eager engine's at index "
                        "%d (%s): %s" % (kind.name, prev, len(self.history), self.graphs, diff[0], diff[1], diff[2],
                                         self.classify()))
        new_slot = ms.per_slot(kind) and (kind.name, self.slot) not in self.seen
        if ms.per_slot(kind):
            self.seen.add((kind.name, self.slot))
        self.slot = (self.slot + ms.slot_advance(kind)) % ms.SLOTS
        if replay and self.graphs:
            assert growth == (1 if new_slot else 0), \
                "%s (after %s): graphs_cached moved by %d on a visit that must replay" % (kind.name, prev, growth)
        if not self.graphs:
            assert growth == 0 and before == 0
        return growth

    def classify(self):
        """The same calls on an engine without graphs tell a key or invalidation defect from a state leak."""
        if not self.graphs:
            return "no graph is involved: one mode leaves state behind for the next"
        eng = self.w.engine(False)
        try:
            for kind in self.history:
                got = self.w.run(eng, kind)
        finally:
            eng.close()
        if ms.first_difference(got, self.w.expected(self.history[-1])) is None:
            return "the same calls WITHOUT graphs give the reference: a graph key or an invalidation defect"
        return "the same calls without graphs fail too: a state leak between modes, not a graph defect"


def orders(kinds, seed=20):
    o1 = [k for k in kinds for _ in range(2)]
    o2 = list(kinds)
    random.Random(seed).shuffle(o2)
    return o1, o2, o1[::-1]


def kinds_of(family):
    return ms.family(family)


@pytest.mark.parametrize("family", ms.FAMILIES)
def test_reference_is_stable_run_to_run(world, family):
    kind = ms.KINDS[STABLE[family]]
    diff = ms.first_difference(world.fresh(kind), world.expected(kind))
    assert diff is None, "%s on two fresh eager engines: field %s, index %d: %s" % ((kind.name,) + diff)


def test_reference_results_are_what_the_table_says(world):
    """The conditions the schedule rests on, on the engine's own references: the fall-back retries, the seeking call
    crosses three windows, a clip of the stop_at_eot kinds stops early, best-of keeps a sample other than the first."""
    import numpy as np
    info = world.expected(ms.KINDS["full40/fallback"])["decode_info"]
    attempts = np.frombuffer(info[3], world.pkg.DECODE_DTYPE)["attempts"]
    print("fall-back attempts per clip:", attempts.tolist())
    assert attempts.max() > 1
    windows = world.expected(ms.SEEK)["windows"]
    assert windows[1][0] >= ms.SEEK_WINDOWS
    for name, cap in (("short/default", 31), ("full40/plain", ms.P_SHORT + 1)):
        assert ms.ids_of(world.expected(ms.KINDS[name]))[1].min() < cap
    picked = world.expected(ms.KINDS["wide/best_of3"])["best_of[0]"]
    assert np.frombuffer(picked[3], np.int32).max() > 0


@pytest.mark.parametrize("family", ms.FAMILIES)
def test_schedule_on_one_engine_with_graphs(world, family):
    o1, o2, o3 = orders(kinds_of(family))
    v = Visits(world)
    try:
        for i, kind in enumerate(o1):      # eager + capture, then the replay
            v.visit(kind, replay=i % 2 == 1)
        held = v.cached()
        for kind in o2 + o3:
            v.visit(kind, replay=True)
        print("%s: %d calls, graphs_cached %d after the first part, %d at the end" % (family, len(v.history), held, v.cached()))
        assert v.eng.get_option("use_graphs") == 1   # a failed capture switches the graphs off: the test would be vacuous
        assert held > 0 or not any(ms.key_families(k) for k in o2)
    finally:
        v.close()


@pytest.mark.parametrize("family", ms.FAMILIES)
def test_schedule_on_one_engine_without_graphs(world, family):
    _, o2, _ = orders(kinds_of(family))
    v = Visits(world, graphs=False)
    try:
        for kind in o2:
            v.visit(kind)
    finally:
        v.close()


def test_neighbour_pairs(world):
    for a, b, setting in ms.NEIGHBOURS:
        diff = ms.first_difference(world.expected(ms.KINDS[a]), world.expected(ms.KINDS[b]))
        assert diff is not None, "%s and %s (%s) give one result: a stale replay across them would go unseen" % (a, b, setting)
    v = Visits(world)
    try:
        for a, b, setting in ms.NEIGHBOURS + ms.ARRANGEMENTS:
            ka, kb = ms.KINDS[a], ms.KINDS[b]
            for kind in (ka, ka, kb, kb, ka, kb):
                v.visit(kind)
        assert v.eng.get_option("use_graphs") == 1
    finally:
        v.close()
    for a, b, setting in ms.ARRANGEMENTS:   # reported, not asserted: the arrangement of the arithmetic alone
        same = ms.first_difference(world.expected(ms.KINDS[a]), world.expected(ms.KINDS[b])) is None
        print("arrangement pair %s / %s (%s): %s" % (a, b, setting, "identical bits" if same else "differed"))


def test_reallocations_destroy_exactly_their_graphs(world):
    two = [ms.KINDS[n] for n in ("short/default", "short/beam2", "full40/ts", "full40/plain", "wide/beam2", "wide/best_of3")]
    assert {f for k in two for f in ms.key_families(k)} == {"greedy", "beam", "full", "beam_full", "best_of"}
    v = Visits(world, warm=False)
    try:
        first = {k.name: v.visit(k) for k in two}
        assert all(g > 0 for g in first.values()), first
        # a 31-position call at 6 clips: the workspace grows and EVERY graph goes; what is left is what that call captured
        assert v.visit(WARM) == first["short/default"] - sum(first.values())
        assert v.cached() == first["short/default"]
        again = {k.name: v.visit(k) for k in two}   # each captures again, and gives the reference
        assert again == first
        # a full-length call at 6 clips after those at 2: the self-attention cache grows, the full-length greedy graphs go,
        # the beam, best-of and 31-position ones stay.  stop_at_eot = 0: the chain runs both of its segments whatever the
        # clips do, so the call captures exactly two graphs.
        full = sum(g for name, g in again.items() if ms.key_families(ms.KINDS[name]) == ("full",))
        assert v.visit(ms.with_clips(ms.KINDS["full40/no_eot"], ms.C6)) == 2 - full
        third = {k.name: v.visit(k) for k in two}
        for k in two:
            gone = ms.key_families(k) == ("full",) or ms.per_slot(k)   # (31-position beam search: the next slot's graph)
            assert third[k.name] == (again[k.name] if gone else 0), (k.name, third, again)
        assert v.eng.get_option("use_graphs") == 1
    finally:
        v.close()


def test_cross_family_interleaving(world):
    names = ("short/default", "short/beam4", "full40/ts_scores", "full40/suppress_l1", "full96/temp_seed_a", "full96/words",
             "wide/beam3", "wide/best_of3_ts", "seek/long")
    order = [ms.KINDS[n] for n in names] * 3
    random.Random(5).shuffle(order)
    v = Visits(world)
    try:
        for kind in order:   # a kind's first visit runs eagerly and captures, every later one must replay
            v.visit(kind, replay=kind in v.history)
        assert v.eng.get_option("use_graphs") == 1
    finally:
        v.close()
