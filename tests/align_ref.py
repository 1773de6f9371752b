"""TEST INFRASTRUCTURE: the restatement of word-level timestamps in numpy and plain Python, what
openai-whisper's timing.py find_alignment() and merge_punctuations() and its tokenizer's split_to_word_tokens() compute,
with the departures the design names.  The continuous stages (column statistics, median filter, head mean) are float64;
the dynamic time warping is fp32 with the one recurrence the engine uses, so that it is defined to the bit; the word
rules work on the vocabulary's bytes."""
import string

import numpy as np

FRAME_MS = 20
UNICODE_ONLY_LANGUAGES = ("zh", "ja", "th", "lo", "my", "yue")
PREPEND = "\"'\u201c\u00bf([{-"
APPEND = "\"'.\u3002,\uff0c!\uff01?\uff1f:\uff1a\u201d)]}\u3001"
ASCII_SPACE = b" \t\n\r\x0b\x0c"


# ------------------------------------------------------------------ DTW ---
def _trace_code(c0, c1, c2):
    """The step the back-trace takes; the COST a cell adds is min(c0, c1, c2) whatever the code says (on c0 == c1 < c2 the
    code is 2 although c2 is not the minimum)."""
    if c0 < c1 and c0 < c2:
        return 0
    if c1 < c0 and c1 < c2:
        return 1
    return 2


def backtrace(trace):
    """trace [N + 1][F + 1] codes (border included) -> path [(row, frame)] from (0, 0) on."""
    trace = trace.copy()
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = trace.shape[0] - 1, trace.shape[1] - 1
    back = []
    while i > 0 or j > 0:
        if i > 0 and j > 0:  # with finite costs the walk meets the border at (0, 0) only
            back.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return back[::-1]


def jump_of(path, N):
    jump = np.zeros(N, np.int32)
    seen = set()
    for r, t in path:
        if r not in seen:
            seen.add(r)
            jump[r] = t
    return jump


def dtw_plain(C):
    """The recurrence cell by cell, row-major: D[i][j] = C[i - 1][j - 1] + min(c0, c1, c2) in fp32."""
    C = np.asarray(C, np.float32)
    N, F = C.shape
    D = np.full((N + 1, F + 1), np.inf, np.float32)
    D[0, 0] = 0
    trace = np.full((N + 1, F + 1), 2, np.uint8)
    for i in range(1, N + 1):
        for j in range(1, F + 1):
            c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
            t = _trace_code(c0, c1, c2)
            D[i, j] = np.float32(C[i - 1, j - 1]) + np.float32(min(c0, c1, c2))
            trace[i, j] = t
    path = backtrace(trace)
    return jump_of(path, N), path, trace[1:, 1:].copy(), D


def dtw(C):
    """The same recurrence swept by anti-diagonals (every cell of one depends on the two before it only), which numpy
    does a diagonal at a time: each cell is still ONE fp32 add of a minimum, so the bits are dtw_plain's.
    Returns (jump int32 [N], path, trace uint8 [N][F], D float32 [N + 1][F + 1])."""
    C = np.ascontiguousarray(C, np.float32)
    N, F = C.shape
    D = np.full((N + 1, F + 1), np.inf, np.float32)
    D[0, 0] = 0
    trace = np.full((N + 1, F + 1), 2, np.uint8)
    for k in range(2, N + F + 1):
        i = np.arange(max(1, k - F), min(N, k - 1) + 1)
        j = k - i
        c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2)).astype(np.uint8)
        c = np.minimum(np.minimum(c0, c1), c2)
        D[i, j] = C[i - 1, j - 1] + c
        trace[i, j] = t
    path = backtrace(trace)
    return jump_of(path, N), path, trace[1:, 1:].copy(), D


def dtw_cases():
    """The matrices the host function and the kernel are both held to: [(name, C float32 [N][F])]."""
    rng = np.random.default_rng(2101)
    cases = [("n1", rng.standard_normal((1, 9))), ("f1", rng.standard_normal((6, 1))), ("one_cell", rng.standard_normal((1, 1))),
             ("n_above_f", rng.standard_normal((40, 7))), ("n2_f3", rng.standard_normal((2, 3))),
             ("all_equal", np.full((9, 13), 0.25)), ("all_zero", np.zeros((5, 4))),
             ("full", rng.standard_normal((447, 1500)))]
    stairs = np.ones((12, 40))  # a planted staircase with a wide margin: row r sits on frames 3 r .. 3 r + 2, then the tail
    for r in range(12):
        stairs[r, 3 * r:3 * r + 3] = -5.0
    stairs[11, 36:] = -5.0
    cases.append(("staircase", stairs))
    signed = rng.integers(-1, 2, (17, 23)).astype(np.float32)  # -1, 0, 1 with many equal neighbours, zeros of both signs
    signed[signed == 0] = np.where(rng.random(int((signed == 0).sum())) < 0.5, -0.0, 0.0)
    cases.append(("signed_zero", signed))
    for k in range(500):
        N, F = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        if k % 3 == 0:
            C = rng.integers(0, 3, (N, F)).astype(np.float32)  # few values: ties everywhere
        else:
            C = rng.standard_normal((N, F))
        cases.append((f"seeded{k}", C))
    return [(name, np.ascontiguousarray(C, np.float32)) for name, C in cases]


# --------------------------------------------------------- cost matrix ---
def column_stats(W, L, F):
    """W [heads][>= L][>= F] of ONE clip -> (mean, rstd) float64 [heads][F] over the L fed positions (population
    statistics); a column of equal values has rstd = 0."""
    X = np.asarray(W, np.float64)[:, :L, :F]
    mean = X.mean(axis=1)
    equal = X.max(axis=1) == X.min(axis=1)
    std = np.sqrt(((X - mean[:, None, :]) ** 2).mean(axis=1))
    rstd = np.where(equal, 0.0, 1.0 / np.where(equal, 1.0, std))
    return mean, rstd


def cost_matrix(W, L, F, n_a):
    """W [heads][>= L][>= F] of ONE clip -> C float64 [L - n_a - 1][F]: normalise every column over the positions,
    median of 7 along the frames with reflect padding (skipped when F <= 3), mean over the heads, negate, keep the rows
    of <|notimestamps|> and of the text ids."""
    X = np.asarray(W, np.float64)[:, :L, :F]
    mean, rstd = column_stats(W, L, F)
    Z = (X - mean[:, None, :]) * rstd[:, None, :]
    if F > 3:
        Zp = np.pad(Z, ((0, 0), (0, 0), (3, 3)), mode="reflect")
        Z = np.median(np.lib.stride_tricks.sliding_window_view(Zp, 7, axis=2), axis=-1)
    return -Z[:, n_a:L - 1, :].mean(axis=0)


# --------------------------------------------------------------- words ---
def _decode(b):
    return bytes(b).decode("utf-8", "replace")


def split_unicode(toks):
    """toks: the bytes of every id of the row -> id counts of the groups that decode to complete characters."""
    full = _decode(b"".join(toks))
    groups, cur, count, offset = [], b"", 0, 0
    for t in toks:
        cur += t
        count += 1
        dec = _decode(cur)
        at = dec.find("\ufffd")
        if at < 0 or (offset + at < len(full) and full[offset + at] == "\ufffd"):
            groups.append(count)
            offset += len(dec)
            cur, count = b"", 0
    if count:
        groups.append(count)
    return groups


def split_words(toks, ids, eot, unicode_only=False):
    groups = split_unicode(toks)
    if unicode_only:
        return groups
    words, at = [], 0
    for n in groups:
        text = b"".join(toks[at:at + n])
        core = text.strip(ASCII_SPACE)
        special = ids[at] >= eot
        with_space = text.startswith(b" ")
        punctuation = len(core) == 1 and chr(core[0]) in string.punctuation
        if special or with_space or punctuation or not words:
            words.append(n)
        else:
            words[-1] += n
        at += n
    return words


def merge_punctuation(toks, word_len):
    prepend = [c.encode() for c in PREPEND]
    append = [c.encode() for c in APPEND]
    words, at = [], 0
    for n in word_len:
        words.append([b"".join(toks[at:at + n]), n])
        at += n
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        prev, nxt = words[i], words[j]
        if prev[0].startswith(b" ") and prev[0].strip(ASCII_SPACE) in prepend:
            nxt[0], nxt[1] = prev[0] + nxt[0], prev[1] + nxt[1]
            prev[0], prev[1] = b"", 0
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        prev, nxt = words[i], words[j]
        if not prev[0].endswith(b" ") and nxt[0] in append:
            prev[0], prev[1] = prev[0] + nxt[0], prev[1] + nxt[1]
            nxt[0], nxt[1] = b"", 0
        else:
            i = j
        j += 1
    return [n for _, n in words if n]


# ------------------------------------------------- float64 decoder forward ---
def _ln(x, g, b):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * g + b


def _erf(x):
    from math import erf
    return np.vectorize(erf, otypes=[np.float64])(x)


def decoder_forward(dims, tensors, row, enc):
    """Whisper's text decoder on ONE id row, teacher-forced, in float64: token + positional embedding, pre-LN blocks
    (causal self-attention, cross-attention over all of enc [T][d], erf-GELU MLP), final LayerNorm and the tied logits.
    Returns (logits [L][n_vocab], qk: {(layer, head): cross-attention scores [L][T] in log2 units, i.e. q . k / 8 times
    log2 e}), the scores Whisper keeps as QKs."""
    t = {k: np.asarray(v, np.float64) for k, v in tensors.items() if k.startswith("decoder.")}
    H, d = dims["n_text_head"], dims["n_text_state"]
    L = len(row)
    enc = np.asarray(enc, np.float64)
    x = t["decoder.token_embedding.weight"][np.asarray(row)] + t["decoder.positional_embedding"][:L]
    causal = np.triu(np.ones((L, L), bool), 1)
    qk = {}
    for l in range(dims["n_text_layer"]):
        blk = f"decoder.blocks.{l}"
        h = _ln(x, t[blk + ".attn_ln.weight"], t[blk + ".attn_ln.bias"])
        q = h @ t[blk + ".attn.query.weight"].T + t[blk + ".attn.query.bias"]
        k = h @ t[blk + ".attn.key.weight"].T
        v = h @ t[blk + ".attn.value.weight"].T + t[blk + ".attn.value.bias"]
        att = np.zeros_like(x)
        for hh in range(H):
            s = slice(64 * hh, 64 * hh + 64)
            sc = q[:, s] @ k[:, s].T / 8.0
            sc[causal] = -np.inf
            p = np.exp(sc - sc.max(axis=-1, keepdims=True))
            att[:, s] = (p / p.sum(axis=-1, keepdims=True)) @ v[:, s]
        x = x + att @ t[blk + ".attn.out.weight"].T + t[blk + ".attn.out.bias"]
        h = _ln(x, t[blk + ".cross_attn_ln.weight"], t[blk + ".cross_attn_ln.bias"])
        q = h @ t[blk + ".cross_attn.query.weight"].T + t[blk + ".cross_attn.query.bias"]
        k = enc @ t[blk + ".cross_attn.key.weight"].T
        v = enc @ t[blk + ".cross_attn.value.weight"].T + t[blk + ".cross_attn.value.bias"]
        att = np.zeros_like(x)
        for hh in range(H):
            s = slice(64 * hh, 64 * hh + 64)
            sc = q[:, s] @ k[:, s].T / 8.0
            qk[(l, hh)] = sc * np.log2(np.e)
            p = np.exp(sc - sc.max(axis=-1, keepdims=True))
            att[:, s] = (p / p.sum(axis=-1, keepdims=True)) @ v[:, s]
        x = x + att @ t[blk + ".cross_attn.out.weight"].T + t[blk + ".cross_attn.out.bias"]
        h = _ln(x, t[blk + ".mlp_ln.weight"], t[blk + ".mlp_ln.bias"])
        h = h @ t[blk + ".mlp.0.weight"].T + t[blk + ".mlp.0.bias"]
        h = 0.5 * h * (1.0 + _erf(h / np.sqrt(2.0)))
        x = x + h @ t[blk + ".mlp.2.weight"].T + t[blk + ".mlp.2.bias"]
    x = _ln(x, t["decoder.ln.weight"], t["decoder.ln.bias"])
    return x @ t["decoder.token_embedding.weight"].T, qk


def default_heads(dims):
    return [(l, h) for l in range(dims["n_text_layer"] // 2, dims["n_text_layer"]) for h in range(dims["n_text_head"])]


def weights(dims, tensors, row, enc, heads, F):
    """W float64 [heads][L][T]: the softmax over the frames t < F of the alignment heads' scores, zero behind."""
    _, qk = decoder_forward(dims, tensors, row, enc)
    W = np.zeros((len(heads), len(row), enc.shape[0]))
    for a, lh in enumerate(sorted(heads)):
        s = qk[lh][:, :F]
        p = np.exp2(s - s.max(axis=-1, keepdims=True))
        W[a, :, :F] = p / p.sum(axis=-1, keepdims=True)
    return W


def words(toks, ids, eot, jump, unicode_only=False):
    """text ids + [eot] (toks their bytes) and jump [n_text + 1] -> [(first text index, id count, t0_ms, t1_ms)] of the
    merged words; the final EOT word only lends its start as the last end time."""
    n_text = len(ids) - 1
    split = split_words(toks, ids, eot, unicode_only)
    kept, covered = [], 0
    for n in split:
        n = min(n, n_text - covered)
        if n > 0:
            kept.append(n)
        covered += n
    out, s0 = [], 0
    for n in merge_punctuation(toks[:n_text], kept):
        out.append((s0, n, int(jump[s0]) * FRAME_MS, int(jump[s0 + n]) * FRAME_MS))
        s0 += n
    return out
