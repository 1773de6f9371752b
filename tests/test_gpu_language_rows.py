"""language_head_rows (k_misc.hip) alone through its tap, against float64 numpy: the language head on
16-lane groups with its candidate mask, per-clip holds, row mapping and fan-out over up to two id tables.  The idioms
are those of test_gpu_language.py: NaN rows around the language rows of the table, guard columns and rows in the id
tables.  Without the kernel the tap does not exist, so every test here fails."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lang_model as lm  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
# the project's bar for a language probability against float64 at d <= 384 (test_gpu_language.py).  Nothing was
# measured at d = 1280: there the bar is the larger of this and twice what language_head shows on the same case
# through its own tap (the factor covers the other partial-sum order of 16-lane groups).
# Measured largest |p - p64| over every case of test_kernel_against_float64 and test_masks: see DESIGN section 32.
KERNEL_P_TOL = 6e-7
LANG_LO_TAP = 7  # the tap's table: rows before and after the language rows hold NaN
GUARD = -77


def code_of(exc):
    return {"WT_ERR_UNSUPPORTED": 4, "WT_ERR_INVALID_ARG": INVALID}.get(str(exc.value).split(":")[0])


@pytest.fixture(scope="module")
def tap_eng(pkg, assets):
    prefix, vocab = assets("micro")
    eng = pkg.Engine(prefix, vocab, True)
    yield eng
    eng.close()


def head_case(d, n_lang, x_rows, part, seed=0):
    """x [x_rows][d] (+ xpart), LayerNorm weights and a table whose non-language rows are NaN."""
    rng = np.random.default_rng(1000 * d + 10 * n_lang + x_rows + (5 if part else 0) + seed)
    x = (rng.standard_normal((x_rows, d)) * 1.5 + 0.3).astype(np.float32)
    xp = (rng.standard_normal((x_rows, d)) * 0.5).astype(np.float32) if part else None
    g = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    E = np.full((LANG_LO_TAP + n_lang + 2, d), np.nan, np.float32)
    E[LANG_LO_TAP:LANG_LO_TAP + n_lang] = (rng.standard_normal((n_lang, d)) * 2.0 / np.sqrt(d)).astype(np.float32)
    return x, xp, g, b, E


def logits64(x, xp, g, b, E, n_lang):
    r = x.astype(np.float64) + (xp.astype(np.float64) if xp is not None else 0.0)
    mu = r.mean(axis=1, keepdims=True)
    var = ((r - mu) ** 2).mean(axis=1, keepdims=True)
    y = (r - mu) / np.sqrt(var + 1e-5) * g.astype(np.float64) + b.astype(np.float64)
    return y @ E[LANG_LO_TAP:LANG_LO_TAP + n_lang].astype(np.float64).T


def masked_ref(z, allowed):
    """float64 probabilities over the allowed languages (exactly 0 elsewhere), the argmax (larger id on a tie) and the
    top-two gap among the allowed."""
    idx = np.nonzero(allowed)[0]
    p = np.zeros(len(z))
    p[idx] = lm.softmax64(z[idx])
    zz = z[idx]
    top = idx[len(zz) - 1 - int(np.argmax(zz[::-1]))]
    gap = float(np.sort(zz)[-1] - np.sort(zz)[-2]) if len(zz) > 1 else np.inf
    return p, int(top), gap


def words_of(allowed):
    w = np.zeros(4, np.uint32)
    for r in np.nonzero(allowed)[0]:
        w[r >> 5] |= np.uint32(1 << (r & 31))
    return w


def id_tables(clips, fan, stride, n):
    """n tables with one guard row in front and two behind the clips * fan rows in use."""
    rows = 1 + clips * fan + 2
    return [np.arange(rows * stride, dtype=np.int64).reshape(rows, stride) + 1000 * (t + 1) for t in range(n)]


def check_id_writes(before, after, clips, fan, id_pos, lang):
    """Only column id_pos of rows [0, clips * fan) changes: row b * fan + j holds LANG_LO_TAP + lang[b]."""
    want = before.copy()
    for b in range(clips):
        want[b * fan:(b + 1) * fan, id_pos] = LANG_LO_TAP + int(lang[b])
    assert np.array_equal(after, want)


# ------------------------------------------------------------------------------------ shapes against float64 ---

@pytest.mark.parametrize("n_lang", [1, 5, 16, 17, 99])  # the group-count edges: one row, under, at and over 16, seven rounds
@pytest.mark.parametrize("d", [64, 128, 384, 1280])
def test_kernel_against_float64(tap_eng, d, n_lang):
    worst = 0.0
    for clips in (1, 3):
        for rpc in (1, 5):
            for part in (False, True):
                for fan, n_tab in ((1, 1), (5, 2), (5, 1), (1, 2)):
                    x_rows = (clips - 1) * rpc + 1
                    x, xp, g, b, E = head_case(d, n_lang, x_rows, part, seed=rpc)
                    # rows of x that no clip reads hold NaN
                    used = np.zeros(x_rows, bool)
                    used[::rpc] = True
                    x[~used] = np.nan
                    tabs = id_tables(clips, fan, 6, n_tab)
                    views = [t[1:] for t in tabs]  # the tap sees the table from its second row: the first is a guard
                    probs, lang, prob, o0, o1 = tap_eng.dbg_language_head_rows(
                        x, g, b, E, LANG_LO_TAP, n_lang, clips, rpc, xpart=xp, ids=views[0],
                        ids2=views[1] if n_tab == 2 else None, id_pos=2, fan=fan)
                    xs, xps = x[::rpc][:clips], (xp[::rpc][:clips] if part else None)
                    z = logits64(xs, xps, g, b, E, n_lang)
                    want = np.stack([lm.softmax64(zz) for zz in z])
                    err = float(np.abs(probs.astype(np.float64) - want).max())
                    old = tap_eng.dbg_language_head(xs, g, b, E, LANG_LO_TAP, n_lang, xpart=xps)
                    err_old = float(np.abs(old[0].astype(np.float64) - want).max())
                    bar = KERNEL_P_TOL if d <= 384 else max(KERNEL_P_TOL, 2.0 * err_old)
                    print(f"d {d} n_lang {n_lang} clips {clips} rpc {rpc} part {part} fan {fan} tables {n_tab}: "
                          f"max |p - p64| = {err:.3e} (language_head {err_old:.3e}, bar {bar:.3e})")
                    worst = max(worst, err)
                    assert np.all(np.isfinite(probs))
                    assert err <= bar
                    assert np.all(np.abs(probs.astype(np.float64).sum(axis=1) - 1.0) <= 1e-5)
                    assert np.array_equal(lang, old[1])  # without mask or hold: language_head's language
                    for r in range(clips):
                        if n_lang > 1 and lm.top_two_gap(z[r]) > 1e-4:
                            assert lang[r] == lm.argmax_last(z[r])
                        assert prob[r] == probs[r, lang[r]]
                    for t, out in zip(views, (o0, o1)):
                        check_id_writes(t, out, clips, fan, 2, lang)
    print(f"d {d} n_lang {n_lang}: largest error {worst:.3e}")


# ------------------------------------------------------------------------------------------------- masks ---

def mask_cases(n_lang, z_row):
    top = int(np.argmax(z_row))
    yield "all", np.ones(n_lang, bool)
    one = np.zeros(n_lang, bool)
    one[n_lang // 3] = True
    yield "one", one
    alt = np.zeros(n_lang, bool)
    alt[::2] = True
    yield "alternating", alt
    last = np.zeros(n_lang, bool)
    last[n_lang - 1] = True
    yield "last", last
    no_top = np.ones(n_lang, bool)
    no_top[top] = False
    yield "without the unmasked argmax", no_top


@pytest.mark.parametrize("d,n_lang", [(128, 99), (384, 17), (64, 5), (1280, 99)])
def test_masks(tap_eng, d, n_lang):
    clips = 3
    x, xp, g, b, E = head_case(d, n_lang, clips, True, seed=3)
    z = logits64(x, xp, g, b, E, n_lang)
    free = tap_eng.dbg_language_head_rows(x, g, b, E, LANG_LO_TAP, n_lang, clips, xpart=xp)
    old = tap_eng.dbg_language_head(x, g, b, E, LANG_LO_TAP, n_lang, xpart=xp)
    err_old = float(np.abs(old[0].astype(np.float64) - np.stack([lm.softmax64(zz) for zz in z])).max())
    bar = KERNEL_P_TOL if d <= 384 else max(KERNEL_P_TOL, 2.0 * err_old)
    for name, allowed in mask_cases(n_lang, z[0]):
        w = words_of(allowed)
        w[3] |= np.uint32(0xF0000000)  # bits at and above n_lang are not languages: they change nothing
        probs, lang, prob, _, _ = tap_eng.dbg_language_head_rows(x, g, b, E, LANG_LO_TAP, n_lang, clips, xpart=xp, allow=w)
        worst = 0.0
        for r in range(clips):
            want, top, gap = masked_ref(z[r], allowed)
            worst = max(worst, float(np.abs(probs[r].astype(np.float64) - want).max()))
            assert np.all(probs[r][~allowed] == 0.0)  # exactly
            assert abs(float(probs[r].astype(np.float64).sum()) - 1.0) <= 1e-5
            assert allowed[lang[r]]
            if gap > 1e-4:
                assert lang[r] == top, (name, r, gap)
            assert prob[r] == probs[r, lang[r]]
        print(f"d {d} n_lang {n_lang} mask {name}: max |p - p64| = {worst:.3e} (bar {bar:.3e})")
        assert worst <= bar
        if name == "all":  # the full mask is no mask, bit for bit
            assert probs.tobytes() == free[0].tobytes() and np.array_equal(lang, free[1]) and prob.tobytes() == free[2].tobytes()
        if name == "one":
            assert np.all(probs[:, n_lang // 3] == 1.0) and np.all(lang == n_lang // 3) and np.all(prob == 1.0)
        if name == "without the unmasked argmax":
            assert lang[0] != free[1][0]


# ------------------------------------------------------------------------------------------------- holds ---

def test_holds_mix_with_detection_in_one_launch(tap_eng):
    n_lang, clips = 99, 4
    x, xp, g, b, E = head_case(128, n_lang, clips, False, seed=11)
    free = tap_eng.dbg_language_head_rows(x, g, b, E, LANG_LO_TAP, n_lang, clips)
    hold = np.array([-1, 41, 1000, 0], np.int32)  # detect, fixed, past the range (clamped), fixed at 0
    tabs = id_tables(clips, 2, 5, 1)
    probs, lang, prob, o0, _ = tap_eng.dbg_language_head_rows(x, g, b, E, LANG_LO_TAP, n_lang, clips, hold=hold, ids=tabs[0][1:],
                                                              id_pos=4, fan=2)
    assert probs.tobytes() == free[0].tobytes()  # a hold leaves the probabilities the detected ones
    assert list(lang) == [int(free[1][0]), 41, n_lang - 1, 0]
    assert np.array_equal(prob, probs[np.arange(clips), lang])
    check_id_writes(tabs[0][1:], o0, clips, 2, 4, lang)
    # a held language outside the mask is still reported, with probability 0
    allowed = np.ones(n_lang, bool)
    allowed[41] = False
    p2, l2, q2, _, _ = tap_eng.dbg_language_head_rows(x, g, b, E, LANG_LO_TAP, n_lang, clips, hold=hold, allow=words_of(allowed))
    assert l2[1] == 41 and q2[1] == 0.0 and p2[1, 41] == 0.0 and allowed[l2[0]]


# -------------------------------------------------------------------------------------------------- ties ---

# group g of 16 lanes takes rows g, g + 16, ...; round k holds rows 16 k .. 16 k + 15; the softmax wavefront's lane l
# owns entries l and l + 64.  (3, 19): one group, two rounds; (3, 4): neighbouring groups of one wavefront, one round;
# (3, 12): groups of different wavefronts, one round; (2, 66): one softmax lane; (97, 98) and (0, 98): across rounds
@pytest.mark.parametrize("d,n_lang,pair", [(128, 99, (3, 19)), (128, 99, (3, 4)), (384, 99, (3, 12)), (128, 99, (2, 66)),
                                           (1280, 99, (97, 98)), (128, 99, (0, 98)), (64, 5, (1, 4)), (64, 17, (0, 16))])
def test_ties_go_to_the_larger_allowed_id(tap_eng, d, n_lang, pair):
    x, xp, g, b, E = head_case(d, n_lang, 2, False, seed=77)
    z = logits64(x, xp, g, b, E, n_lang)
    lo, hi = pair
    for r in range(2):
        Er = E.copy()
        top = int(np.argmax(z[r]))
        assert z[r][top] > 0
        Er[LANG_LO_TAP + lo] = Er[LANG_LO_TAP + hi] = 1.5 * E[LANG_LO_TAP + top]
        tabs = id_tables(2, 1, 4, 1)
        probs, lang, prob, o0, _ = tap_eng.dbg_language_head_rows(x, g, b, Er, LANG_LO_TAP, n_lang, 2, ids=tabs[0][1:])
        assert probs[r, lo] == probs[r, hi] and probs[r, hi] == probs[r].max()
        assert lang[r] == hi and o0[r, 1] == LANG_LO_TAP + hi
        # the larger id masked out: the tie's other end is the largest allowed one
        allowed = np.ones(n_lang, bool)
        allowed[hi] = False
        probs, lang, prob, _, _ = tap_eng.dbg_language_head_rows(x, g, b, Er, LANG_LO_TAP, n_lang, 2, allow=words_of(allowed))
        assert lang[r] == lo and probs[r, hi] == 0.0


# ------------------------------------------------------------------------------------------ independence ---

@pytest.mark.parametrize("d,part", [(128, False), (384, True), (1280, True)])
def test_clip_is_independent_of_grid_and_fan(tap_eng, d, part):
    rpc = 5
    x, xp, g, b, E = head_case(d, 99, 2 * rpc + 1, part, seed=5)
    allowed = np.ones(99, bool)
    allowed[::3] = False
    w = words_of(allowed)
    hold = np.array([-1, 7, -1], np.int32)
    t5 = id_tables(3, 5, 4, 1)[0]
    p3, l3, q3, o3, _ = tap_eng.dbg_language_head_rows(x, g, b, E, LANG_LO_TAP, 99, 3, rpc, xpart=xp, allow=w, hold=hold,
                                                       ids=t5[1:], fan=5)
    x1, xp1 = x[2 * rpc:], (xp[2 * rpc:] if part else None)
    t1 = id_tables(1, 1, 4, 1)[0]
    p1, l1, q1, o1, _ = tap_eng.dbg_language_head_rows(x1, g, b, E, LANG_LO_TAP, 99, 1, 1, xpart=xp1, allow=w, ids=t1[1:], fan=1)
    assert p1.tobytes() == p3[2:3].tobytes() and l1[0] == l3[2] and q1.tobytes() == q3[2:3].tobytes()
    assert o1[0, 1] == o3[10, 1] == LANG_LO_TAP + l1[0]
    # fan alone: the same launch with fan 1
    p3b, l3b, q3b, _, _ = tap_eng.dbg_language_head_rows(x, g, b, E, LANG_LO_TAP, 99, 3, rpc, xpart=xp, allow=w, hold=hold,
                                                         ids=id_tables(3, 1, 4, 1)[0][1:], fan=1)
    assert p3b.tobytes() == p3.tobytes() and np.array_equal(l3b, l3) and q3b.tobytes() == q3.tobytes()


# --------------------------------------------------------------------------------------------- refusals ---

def test_launcher_refusals(pkg, tap_eng):
    n_lang, clips = 99, 3
    x, xp, g, b, E = head_case(128, n_lang, 11, False, seed=9)
    tab = id_tables(clips, 2, 4, 1)[0][1:]  # 8 rows, 6 of them in use at fan 2

    def call(**kw):
        a = {"lang_lo": LANG_LO_TAP, "n_lang": n_lang, "clips": clips, "rpc": 5, "ids": tab, "id_pos": 1, "fan": 2, "x": x, "g": g,
             "b": b, "E": E}
        a.update(kw)
        return tap_eng.dbg_language_head_rows(a["x"], a["g"], a["b"], a["E"], a["lang_lo"], a["n_lang"], a["clips"], a["rpc"],
                                              ids=a["ids"], id_pos=a["id_pos"], fan=a["fan"])

    good = call()
    assert np.all(np.isfinite(good[0]))
    d126 = head_case(126, n_lang, 11, False)
    d1284 = head_case(1284, n_lang, 11, False)
    bad = [{"x": d126[0], "g": d126[2], "b": d126[3], "E": d126[4]},  # d % 4
           {"x": d1284[0], "g": d1284[2], "b": d1284[3], "E": d1284[4]},  # d > kLangMaxD
           {"n_lang": 0}, {"n_lang": 129}, {"lang_lo": -1}, {"lang_lo": E.shape[0] - 98},  # ranges
           {"id_pos": 4}, {"id_pos": -1},  # outside the id row
           {"fan": 3}, {"fan": 0}, {"clips": 5, "fan": 2, "rpc": 1},  # id rows that leave the table
           {"rpc": 6}, {"clips": 4}, {"rpc": 0}]  # x rows that leave the buffer
    for kw in bad:
        with pytest.raises(pkg.WtError) as e:
            call(**kw)
        assert code_of(e) == INVALID, kw
    again = call()  # nothing reached the device: the engine is usable and gives the same result
    assert again[0].tobytes() == good[0].tobytes() and np.array_equal(again[3], good[3])
