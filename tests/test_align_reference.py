"""CPU: the host half of word-level timestamps (csrc/words.cpp behind wt_dtw_path,
wt_vocab_split_words and wt_vocab_merge_punctuation) against tests/align_ref.py, and align_ref's own dynamic time warping
against the exhaustive enumeration of monotone paths."""
import ctypes
import os
import string
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_model  # noqa: E402
import align_ref  # noqa: E402

EOT = 50257  # multilingual


# ------------------------------------------------------------------ DTW ---
def _enumerate(C):
    """Every monotone path from (0, 0): best[r][t] = the smallest fp32 sum, added in path order, over the paths that
    end in (r, t).  (D of the recurrence is that minimum: rounding an add is monotone in the addend.)"""
    N, F = C.shape
    best = np.full((N, F), np.inf, np.float32)

    def walk(r, t, acc):
        acc = np.float32(C[r, t]) + acc
        if acc < best[r, t]:
            best[r, t] = acc
        for dr, dt in ((1, 1), (1, 0), (0, 1)):
            if r + dr < N and t + dt < F:
                walk(r + dr, t + dt, acc)

    walk(0, 0, np.float32(0))
    return best


def _path_by_tie_rule(best):
    N, F = best.shape
    D = np.full((N + 1, F + 1), np.inf, np.float32)
    D[0, 0] = 0
    D[1:, 1:] = best
    i, j, back = N, F, []
    while i > 0 and j > 0:
        back.append((i - 1, j - 1))
        t = align_ref._trace_code(D[i - 1, j - 1], D[i - 1, j], D[i, j - 1])
        i, j = (i - 1, j - 1) if t == 0 else (i - 1, j) if t == 1 else (i, j - 1)
    assert (i, j) == (0, 0)
    return back[::-1]


def test_dtw_equals_exhaustive_enumeration():
    rng = np.random.default_rng(77)
    for k in range(200):
        N, F = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        C = (rng.integers(-2, 3, (N, F)) if k % 2 else rng.standard_normal((N, F))).astype(np.float32)
        jump, path, trace, D = align_ref.dtw(C)
        best = _enumerate(C)
        assert D[N, F] == best[N - 1, F - 1]
        assert np.array_equal(D[1:, 1:], best)
        assert path == _path_by_tie_rule(best)
        assert max(N, F) <= len(path) <= N + F - 1
        assert path[0] == (0, 0) and path[-1] == (N - 1, F - 1)
        assert all(jump[r] == min(t for rr, t in path if rr == r) for r in range(N))


def test_diagonal_sweep_equals_the_plain_recurrence():
    for name, C in align_ref.dtw_cases():
        if C.size > 2000:
            continue
        a, b = align_ref.dtw(C), align_ref.dtw_plain(C)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]), name
        assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)), name


def test_planted_staircase_is_found():
    C = dict(align_ref.dtw_cases())["staircase"]
    jump, path, _, D = align_ref.dtw(C)
    assert list(jump) == [3 * r for r in range(12)]
    assert len(path) == 40 and D[12, 40] == -200.0


def test_wt_dtw_path_is_bit_equal_to_the_restatement(pkg):
    for name, C in align_ref.dtw_cases():
        want_jump, want_path, _, _ = align_ref.dtw(C)
        jump, path = pkg.dtw_path(C)
        assert np.array_equal(jump, want_jump), name
        assert [tuple(p) for p in path.tolist()] == want_path, name


def test_wt_dtw_path_arguments(pkg):
    L = pkg.lib()
    C = np.zeros((3, 4), np.float32)
    jump = np.zeros(3, np.int32)
    path = np.full((2, 2), -7, np.int32)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    cp, jp, pp = C.ctypes.data_as(fp), jump.ctypes.data_as(ip), path.ctypes.data_as(ip)
    assert L.wt_dtw_path(cp, 3, 4, jp, pp, 2) == 6  # all ties: along the last row, then up: the count, two pairs written
    assert path.tolist() == [[0, 0], [1, 0]] and list(jump) == [0, 0, 0]
    assert L.wt_dtw_path(cp, 3, 4, jp, None, 0) == 6
    for bad in ((None, 3, 4, jp, None, 0), (cp, 3, 4, None, None, 0), (cp, 0, 4, jp, None, 0), (cp, 3, 0, jp, None, 0),
                (cp, 448, 4, jp, None, 0), (cp, 3, 1501, jp, None, 0), (cp, 3, 4, jp, None, 2), (cp, 3, 4, jp, pp, -1)):
        assert L.wt_dtw_path(*bad) == -1


# ---------------------------------------------------------------- words ---
@pytest.fixture(scope="module")
def hand(pkg, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("align") / "hand_vocab.bin")
    align_model.write_vocab(path)
    v = pkg.Vocab(path, True)
    yield v
    v.close()


def _check_row(v, ids):
    ids = [int(i) for i in ids]
    toks = [v.token(i) for i in ids]
    for unicode_only in (False, True):
        got = v.split_words(ids, unicode_only).tolist()
        want = align_ref.split_words(toks, ids, EOT, unicode_only)
        assert got == want, (ids, unicode_only, got, want)
        assert sum(got) == len(ids) and all(n > 0 for n in got)
        merged = v.merge_punctuation(ids, got).tolist() if ids else []
        want_merged = align_ref.merge_punctuation(toks, want)
        assert merged == want_merged, (ids, unicode_only, merged, want_merged)
        assert sum(merged) == len(ids)
    return v.split_words(ids, False).tolist()


def test_hand_vocabulary_is_what_the_tests_assume(hand):
    for i, t in enumerate(align_model.HAND_TOKENS):
        assert hand.token(i) == t
    assert hand.info()["eot"] == EOT and hand.token(EOT).startswith(b"<|")


def test_split_words_hand_rows(hand):
    P = align_model.PUNCT0
    dot, comma = P + string.punctuation.index("."), P + string.punctuation.index(",")
    # a character over two and over three ids is one group; the words around it are their own
    assert _check_row(hand, [0, 10, 11, 1, EOT]) == [3, 1, 1]            # " hello" + 日 join (no space), " world", eot
    assert hand.split_words([0, 10, 11, 1, EOT], True).tolist() == [1, 2, 1, 1]
    assert hand.split_words([12, 13, 14, 21], True).tolist() == [3, 1]
    assert hand.split_words([16, 17], True).tolist() == [2]
    # a genuine U+FFFD closes its group at once; bytes that never complete close where the row itself has U+FFFD
    assert hand.split_words([15, 4], True).tolist() == [1, 1]
    assert hand.split_words([19, 4, 18, 20], True).tolist() == [1, 1, 1, 1]
    assert hand.split_words([10, 0], True).tolist() == [1, 1]            # two bytes of 日, never its third
    # leading space, continuation, punctuation as its own word, an id >= eot in the middle
    assert _check_row(hand, [0, 2, 3, dot, 1, comma, 4, EOT]) == [3, 1, 1, 2, 1]      # "a" joins the comma's word
    assert _check_row(hand, [0, EOT + 5, 2, 1]) == [1, 2, 1]             # the special id starts a word; "ing" joins it
    assert _check_row(hand, [4, 4, 7, 4]) == [4]                         # "\n" strips to nothing: no punctuation mark
    for k in range(len(string.punctuation)):
        assert _check_row(hand, [0, P + k, 4]) == [1, 2], string.punctuation[k]  # the mark starts a word, "a" joins it
    assert _check_row(hand, []) == []
    assert _check_row(hand, [0]) == [1] and _check_row(hand, [EOT]) == [1] and _check_row(hand, [10]) == [1]


def test_merge_punctuation_hand_rows(pkg, hand):
    P, A0, B0 = align_model.PUNCT0, align_model.PREPEND0, align_model.APPEND0
    dot = P + string.punctuation.index(".")
    merge = lambda ids, words: hand.merge_punctuation(ids, words).tolist()  # noqa: E731
    for k in range(len(align_ref.PREPEND)):  # every leading mark goes in front of the next word
        assert merge([0, A0 + k, 1], [1, 1, 1]) == [1, 2], align_ref.PREPEND[k]
    for k in range(len(align_ref.APPEND)):   # every trailing mark goes behind the word before it
        assert merge([0, B0 + k, 1], [1, 1, 1]) == [2, 1], align_ref.APPEND[k]
    quote_open, paren_open = A0 + align_ref.PREPEND.index('"'), A0 + align_ref.PREPEND.index("(")
    quote_close = B0 + align_ref.APPEND.index('"')
    assert merge([quote_open, 0, quote_close], [1, 1, 1]) == [3]                      # marks at both ends
    assert merge([quote_open, paren_open, 0, dot, quote_close], [1, 1, 1, 1, 1]) == [5]  # two in a row, both sides
    assert merge([0, quote_open], [1, 1]) == [1, 1]                                   # nothing behind it to lead
    assert merge([dot, 0], [1, 1]) == [1, 1]                                          # nothing before it to trail
    assert merge([8, dot], [1, 1]) == [1, 1]                                          # " end " ends in a space
    assert merge([0, P + string.punctuation.index("#")], [1, 1]) == [1, 1]            # not one of the marks
    assert merge([0, 2, dot, 1], [2, 1, 1]) == [3, 1]                                 # words of several ids
    for ids in ([quote_open, 0, quote_close, EOT], [0, dot, dot, quote_close, paren_open, quote_open, 1, EOT], [dot], [quote_open]):
        _check_row(hand, ids)
    hand_lib, L, ip64, ip32 = pkg.lib(), hand._v, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    ids, words, out = np.array([0, 1], np.int64), np.array([1, 2], np.int32), np.zeros(4, np.int32)
    call = lambda n, w, nw: hand_lib.wt_vocab_merge_punctuation(L, ids.ctypes.data_as(ip64), n, w.ctypes.data_as(ip32), nw,  # noqa: E731
                                                                 out.ctypes.data_as(ip32), 4)
    assert call(2, words, 2) == -1                                    # the counts do not add up
    assert call(2, np.array([2, 0], np.int32), 2) == -1               # an empty word
    assert call(2, np.array([1, 1], np.int32), 2) == 2
    assert hand_lib.wt_vocab_split_words(None, ids.ctypes.data_as(ip64), 2, 0, out.ctypes.data_as(ip32), 4) == -1
    assert hand_lib.wt_vocab_split_words(L, ids.ctypes.data_as(ip64), -1, 0, out.ctypes.data_as(ip32), 4) == -1
    out[:] = -7
    assert hand_lib.wt_vocab_split_words(L, ids.ctypes.data_as(ip64), 2, 0, out.ctypes.data_as(ip32), 1) == 2  # the count; one written
    assert out.tolist() == [1, -7, -7, -7]


def test_split_and_merge_seeded_rows_hand_vocabulary(hand):
    rng = np.random.default_rng(5)
    pool = list(range(len(align_model.HAND_TOKENS))) + [EOT, EOT + 1, EOT + 120, 50364, 50400]
    for _ in range(1500):
        n = int(rng.integers(0, 14))
        _check_row(hand, [pool[int(k)] for k in rng.integers(0, len(pool), n)])


def test_split_and_merge_seeded_rows_synthetic_vocabulary(pkg, assets):
    _, vocab = assets("micro")
    v = pkg.Vocab(vocab, True)
    rng = np.random.default_rng(6)
    try:
        for k in range(2000):
            n = int(rng.integers(0, 20))
            ids = np.where(rng.random(n) < 0.6, rng.integers(33, 127, n), rng.integers(0, 50257, n))
            if n and k % 4 == 0:
                ids[-1] = EOT
            if n > 3 and k % 7 == 0:
                ids[int(rng.integers(0, n))] = int(rng.integers(EOT, 51865))
            _check_row(v, ids)
    finally:
        v.close()


def test_decode_with_replacement_follows_python(hand):
    """The group rule leans on Python's decode(errors="replace"): one U+FFFD per maximal ill-formed subpart.  Every
    two- and three-id row over the byte-piece tokens shows whether words.cpp replaces the same way."""
    pieces = list(range(10, 22)) + [4, 0]
    for a in pieces:
        for b in pieces:
            _check_row(hand, [a, b])
            for c in (11, 13, 14, 17, 18, 19, 4):
                _check_row(hand, [a, b, c])


# ------------------------------------------------------ decoder forward ---
def test_float64_decoder_agrees_with_the_oracle(orc, assets, tmp_path):
    """The restatement's decoder (align_ref.decoder_forward) against the CPU oracle's decode_greedy on the timestamp
    model: the logits behind the last id of a teacher-forced row.  The oracle stores fp32 and its logits come
    back as fp32: measured 5.8e-8 of the largest logit (one fp32 rounding is 6e-8), the bar is a decade above."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import ts_model as tm
    from wtw import read_wtw
    prefix, _ = assets("micro")
    path = str(tmp_path / "micro-ts.wtw")
    tm.write_model(prefix + ".wtw", path)
    dims, tensors = read_wtw(path)
    model = orc.Model(path)
    rng = np.random.default_rng(3)
    worst = 0.0
    try:
        for k, mel in enumerate(tm.mels(3)):
            enc = model.encode(mel)
            row = tm.PROMPT + [50363] + [int(i) for i in rng.integers(0, tm.EOT, 5 + 20 * k)] + [tm.EOT]
            _, lg = model.decode_greedy(enc, row, max_positions=len(row), eot=tm.EOT, stop_at_eot=False, want_logits=True)
            logits, qk = align_ref.decoder_forward(dims, tensors, row, enc)
            assert set(qk) == {(l, h) for l in range(dims["n_text_layer"]) for h in range(dims["n_text_head"])}
            err = float(np.abs(logits[-1] - np.asarray(lg[0], np.float64)).max() / np.abs(logits[-1]).max())
            print(f"decoder_forward vs oracle, row of {len(row)}: {err:.3g} of the largest logit")
            worst = max(worst, err)
    finally:
        model.close()
    assert worst <= 6e-7
