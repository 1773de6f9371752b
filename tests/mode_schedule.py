"""The table of decode-call kinds that tests/test_gpu_graph_isolation.py runs against one another on ONE engine, and
tests/test_mode_schedule_reference.py checks on the CPU.

A KIND is a name, an entry point, a clip selection and an option dict.  It is always run as reset(eng), then its
options, then its call, and its RESULT is everything the public surface returns after the call that the entry point
itself defines (a 31-position call leaves the words of an earlier full-length call standing, a
pipelined one also its segments, beam scores and windows, detect_language forgets nothing — GETTERS_OF), each field as
raw bytes, so that NaN and -0 compare; a getter that refuses is recorded as refused.

The model is full_model's EOT-rich flavour over the micro weights (the multilingual vocabulary size, so EOT, timestamp,
<|nospeech|> and language ids all exist; n_text_ctx 160) with flatter text rows and a scaled <|nospeech|> row
(write_model); the clips are tests/scores_model.py's plain ones, the audio of the seeking call is
tests/longform_model.py's.  Nothing in this
module touches the GPU until run() is called."""
from __future__ import annotations

import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

sys.path.insert(0, os.path.join(ROOT, "tools"))

import full_model  # noqa: E402
import longform_model as lm  # noqa: E402
import scores_model  # noqa: E402

RICH = (6.0, 10.0, 64)        # write_eot_rich's eot_gain, gain, n_active
NOSP_GAIN = -250.0            # no_speech_prob of a few 1e-4: compared bit for bit, never against a threshold

EOT, BEG, NOSP = lm.EOT, lm.BEG, lm.NOSP
SOT, LANG_LO, TRANSCRIBE, NOTIMESTAMPS = 50258, 50259, 50359, 50363
PROMPT = [SOT, LANG_LO + 2, TRANSCRIBE, NOTIMESTAMPS]      # the engine's default (language 2)
PROMPT_TS = PROMPT[:3]                                     # ... with timestamps = 1
PROMPT_OTHER_IDS = [SOT, 3, 5, 7]                                 # equal length: device data of a replayed graph
PROMPT_OTHER_LEN = [SOT, LANG_LO + 2, TRANSCRIBE]                # another length: a key entry
P_SHORT, P_LONG = 40, 96      # 40 ends inside the second 32-position segment, 96 makes three segments
SLOTS = 24                    # the engine's pipeline slots: every encoder pass of a 31-position call takes the next one
C2, C4, C6 = (1, 4), (0, 1, 4, 5), (0, 1, 2, 3, 4, 5)   # clips of scores_model.plain_mels()'s twelve
SEED_A, SEED_B = 1, (7 << 32) | 5
TEMP = 700
MAX_INITIAL_OTHER = 0         # <|0.00|> alone may open the row (the default allows 50 ticks)
# Suppression lists, chosen on the CPU from the greedy decode of clips C2 at 40 positions by the rule of
# tests/suppress_model.py: 16 is the text id both clips generate first and most, 50362 what they generate behind L1;
# pinned by tests/test_mode_schedule_reference.py.  L2: L1's counts and other ids (device data); L3: other counts (key
# entries).
L1 = ((0, 16, 51864), (16, 50257))
L2 = ((16, 50362, 51864), (16, 50257))
L3 = ((0, 16, 50362, 51864), (16,))
CONTEXT = tuple(lm.CONTEXT)
CONTEXTS = ((11, 222, 333), ())
# the fall-back of tests/sample_model.py: schedule 0, 0.5, 1.0
FALLBACK = dict(temperature_fallback=1, temperature=0, temperature_increment=500, logprob_threshold=-250,
                compression_ratio_threshold=3000, no_speech_threshold=600, seed=1, scores=1, timestamps=1)

# Every option the table touches and its default (engine.h); reset() writes all of them.
DEFAULTS = dict(
    max_positions=0, timestamps=0, max_initial_timestamp=50, scores=0, skip_silence=0, temperature=0,
    temperature_fallback=0, temperature_increment=200, compression_ratio_threshold=2400, logprob_threshold=-1000,
    no_speech_threshold=600, seed=0, best_of=1, fallback_beam=0, beam_size=1, full_beam=0, seek=0,
    condition_on_previous_text=1, word_timestamps=0, stop_at_eot=1, cross_absorb=1, cross_chunks=0, abs_chunks=0,
    fc2_ksplit=2, max_tokens=30, language=2, bf16=0, suppress_default=0)
# settings that are no numeric option: name -> what reset() puts back
SPECIAL_DEFAULTS = dict(prompt=(), context=(), contexts=(), suppress=((), ()))

Kind = namedtuple("Kind", "name family entry clips options")


def reset(eng):
    """Every option the table touches back to its default; no suppression lists, no context of either kind, the default
    prompt, no forced ids, the default alignment heads and tap settings."""
    for k, v in DEFAULTS.items():
        eng.set_option(k, v)
    eng.set_suppress([], [])
    eng.set_context([])
    eng.set_contexts([])
    eng.set_prompt([])
    eng.set_forced_ids(None)
    eng.set_alignment_heads(())
    eng.dbg_set_alignment(keep=0, mode=1, sub=0)


def apply(eng, options):
    for k, v in options.items():
        if k == "prompt":
            eng.set_prompt(list(v))
        elif k == "context":
            eng.set_context(list(v))
        elif k == "contexts":
            eng.set_contexts([list(c) for c in v])
        elif k == "suppress":
            eng.set_suppress(list(v[0]), list(v[1]))
        else:
            eng.set_option(k, v)


# ---- the kinds --------------------------------------------------------------------------------------------------------
def _short():
    k = lambda name, entry="batch", clips=C2, **o: Kind("short/" + name, "short", entry, clips, o)  # noqa: E731
    return [
        k("default"),
        k("no_eot", stop_at_eot=0),
        k("no_absorb", cross_absorb=0),
        k("no_absorb_chunks4", cross_absorb=0, cross_chunks=4),
        k("ksplit1", fc2_ksplit=1),
        k("ksplit2", fc2_ksplit=2),          # the default, named: shares the default kind's graphs
        k("chunks4", cross_chunks=4),
        k("abs3", abs_chunks=3),
        k("max_tokens12", max_tokens=12),
        k("prompt_ids", prompt=tuple(PROMPT_OTHER_IDS)),
        k("prompt_len", prompt=tuple(PROMPT_OTHER_LEN)),
        k("language_auto", language=-1),
        k("detect", entry="detect"),
        k("beam2", beam_size=2),
        k("beam4", beam_size=4),
        k("bf16", bf16=1),
        k("pipeline2x2", entry="pipeline", clips=C4),   # two batches of two clips from one device buffer
    ]


def _full(P):
    fam = "full%d" % P
    k = lambda name, clips=C2, **o: Kind("%s/%s" % (fam, name), fam, "full", clips, dict(o, max_positions=P))  # noqa: E731
    return [
        k("plain"),
        k("ts", timestamps=1),
        k("ts_initial0", timestamps=1, max_initial_timestamp=MAX_INITIAL_OTHER),
        k("ts_scores", timestamps=1, scores=1),
        k("scores", scores=1),
        k("temp_seed_a", temperature=TEMP, seed=SEED_A),
        k("temp_seed_b", temperature=TEMP, seed=SEED_B),
        k("fallback", **FALLBACK),
        k("suppress_l1", suppress=L1),
        k("suppress_l2", suppress=L2),
        k("suppress_l3", suppress=L3),
        k("suppress_default", suppress_default=1),
        k("context", context=CONTEXT),
        k("contexts", contexts=CONTEXTS),
        k("words", timestamps=1, word_timestamps=1),
        k("no_eot", stop_at_eot=0),
        k("no_absorb", cross_absorb=0),
    ]


def _wide():
    k = lambda name, P=P_SHORT, clips=C2, **o: Kind("wide/" + name, "wide", "full", clips, dict(o, max_positions=P))  # noqa: E731
    return [
        k("beam2", full_beam=1, beam_size=2),
        k("beam3", full_beam=1, beam_size=3),
        k("beam2_long", P=P_LONG, full_beam=1, beam_size=2),
        k("beam2_ts_scores", full_beam=1, beam_size=2, timestamps=1, scores=1),
        k("best_of3", best_of=3, temperature=TEMP, seed=SEED_A),
        k("best_of3_long", P=P_LONG, best_of=3, temperature=TEMP, seed=SEED_A),
        k("best_of3_ts", best_of=3, temperature=TEMP, seed=SEED_A, timestamps=1),
        k("fallback_beam", **dict(FALLBACK, full_beam=1, beam_size=2, fallback_beam=1, best_of=3)),
    ]


SEEK_WINDOWS = 3
SEEK = Kind("seek/long", "seek", "long", (), dict(seek=1, condition_on_previous_text=0, timestamps=1, scores=1,
                                                  max_positions=P_SHORT))
KINDS = {k.name: k for k in _short() + _full(P_SHORT) + _full(P_LONG) + _wide() + [SEEK]}
FAMILIES = ("short", "full40", "full96", "wide", "seek")


def family(name):
    return [k for k in KINDS.values() if k.family == name]


def with_clips(kind, clips):
    """The kind at other clips (the invalidation test's 6-clip calls)."""
    return kind._replace(name="%s@%d" % (kind.name, len(clips)), clips=tuple(clips))


# ---- neighbour pairs --------------------------------------------------------------------------------------------------
# (kind A, kind B, the ONE setting they differ in): the results must differ, or a stale replay across the pair would go
# unseen.  tests/test_mode_schedule_reference.py pins the distinctness on the CPU references where one decodes the pair.
NEIGHBOURS = [
    ("full40/ts", "full40/ts_initial0", "max_initial_timestamp"),
    ("full96/ts", "full96/ts_initial0", "max_initial_timestamp"),
    ("short/default", "short/no_eot", "stop_at_eot"),
    ("full40/plain", "full40/no_eot", "stop_at_eot"),
    ("short/default", "short/prompt_ids", "prompt"),
    ("short/default", "short/prompt_len", "prompt"),
    ("full40/temp_seed_a", "full40/temp_seed_b", "seed"),
    ("full40/suppress_l1", "full40/suppress_l2", "suppress"),
    ("full40/suppress_l1", "full40/suppress_l3", "suppress"),
    ("wide/beam2", "wide/beam3", "beam_size"),
    ("short/beam2", "short/beam4", "beam_size"),
    ("full40/temp_seed_a", "wide/best_of3", "best_of"),
    ("full40/plain", "full40/ts", "timestamps"),
    ("short/default", "short/max_tokens12", "max_tokens"),
]
# Pairs that change the arrangement of the arithmetic alone: they may give identical bits; reported, never asserted.
ARRANGEMENTS = [
    ("short/ksplit2", "short/ksplit1", "fc2_ksplit"),
    ("short/no_absorb", "short/no_absorb_chunks4", "cross_chunks"),
    ("short/default", "short/chunks4", "cross_chunks"),
    ("short/default", "short/abs3", "abs_chunks"),
    ("short/default", "short/no_absorb", "cross_absorb"),
    ("full40/plain", "full40/no_absorb", "cross_absorb"),
]


def settings_of(kind):
    """Every setting of a kind, the defaults filled in."""
    out = dict(DEFAULTS)
    out.update(SPECIAL_DEFAULTS)
    out.update(kind.options)
    return out


def differing(a, b):
    sa, sb = settings_of(a), settings_of(b)
    return sorted(k for k in sa if sa[k] != sb[k])


# ---- the engine's refusal rules, as check_timestamp_call / check_full_call / check_beam_call / check_language_call
# (engine.cpp, engine_full.cpp) state them for this model: the reason a kind would be refused, or None ----------------
def refusal(kind):
    s = settings_of(kind)
    P, K = s["max_positions"], s["beam_size"]
    sampling = s["temperature"] > 0 or s["temperature_fallback"] != 0
    context = bool(s["context"]) or bool(s["contexts"])
    suppressing = bool(s["suppress"][0]) or bool(s["suppress"][1]) or s["suppress_default"] == 1
    full = kind.entry in ("full", "long")
    if full != (P > 0):
        return "max_positions and the entry point disagree"
    if P and not 32 <= P <= full_model.N_TEXT_CTX:
        return "max_positions outside [32, n_text_ctx]"
    for name, on in (("timestamps", s["timestamps"]), ("scores", s["scores"]), ("temperature", sampling),
                     ("seek", s["seek"]), ("context", context), ("suppress", suppressing)):
        if on and P <= 0:
            return name + ": full-length decoding only"
    if s["skip_silence"] and not s["scores"]:
        return "skip_silence needs scores"
    if s["seek"] and not s["timestamps"]:
        return "seek needs timestamps"
    if s["seek"] != (kind.entry == "long"):
        return "seek and the entry point disagree"
    if s["contexts"] and s["word_timestamps"]:
        return "contexts: not with word_timestamps"
    if s["contexts"] and len(s["contexts"]) != len(kind.clips):
        return "contexts: another number of clips"
    if s["word_timestamps"] and (not s["timestamps"] or P <= 0 or not s["cross_absorb"]):
        return "word_timestamps needs timestamps, max_positions and cross_absorb"
    if s["temperature_fallback"] and not s["scores"]:
        return "temperature_fallback needs scores"
    if s["language"] < 0:  # check_language_call
        if K > 1 or s["prompt"]:
            return "automatic language: not with beam search or a caller prompt"
    if K > 1:  # check_beam_call
        if s["bf16"] or not s["cross_absorb"] or not s["stop_at_eot"]:
            return "beam search: not in bf16, needs cross_absorb and stop_at_eot"
    if kind.entry == "pipeline" and (P > 0 or K > 1):
        return "the pipeline takes 31-position greedy calls only"
    if P > 0:  # check_full_call
        if K > 1 and not s["full_beam"]:
            return "full-length: greedy only unless full_beam = 1"
        if s["bf16"] or s["language"] < 0:
            return "full-length: not in bf16, not with language = -1"
        if K > 1:
            fallback_beam = s["fallback_beam"] and s["full_beam"] and sampling
            if sampling and not fallback_beam:
                return "full_beam: not with a temperature"
            if context or s["seek"] or s["word_timestamps"]:
                return "full_beam: not with a context, seek or word_timestamps"
        if s["best_of"] > 1 and sampling:
            if context or s["seek"] or s["word_timestamps"] or not s["stop_at_eot"] or not s["cross_absorb"]:
                return "best_of: not with a context, seek, word_timestamps, stop_at_eot = 0 or cross_absorb = 0"
        n_fed = len(s["prompt"] or (PROMPT_TS if s["timestamps"] else PROMPT))
        longest = max([len(s["context"])] + [len(c) for c in s["contexts"]])
        if context and 1 + longest + n_fed >= P:
            return "context: no position left to generate"
    return None


# ---- which graph keys a kind's chains take -----------------------------------------------------
def key_families(kind):
    s = settings_of(kind)
    if kind.entry in ("batch", "detect", "pipeline"):
        return ("beam",) if s["beam_size"] > 1 else ("greedy",)
    if s["context"] or s["contexts"]:
        return ()  # a context's length is part of every launch: such calls run eagerly
    sampling = s["temperature"] > 0 or s["temperature_fallback"] != 0
    if s["beam_size"] > 1 and not sampling:
        return ("beam_full",)
    out = []
    if s["beam_size"] > 1:
        out.append("beam_full")          # fallback_beam: the attempt at temperature 0
    else:
        out.append("full")               # greedy, or the sampler's one row per clip (an attempt at temperature 0 too)
    if s["best_of"] > 1 and sampling:
        out.append("best_of")
        if s["beam_size"] <= 1 and s["temperature"] > 0 and not s["temperature_fallback"]:
            out.remove("full")           # every attempt is above 0
    return tuple(out)


def per_slot(kind):
    """31-position beam search captures the graph of the slot it runs in alone (greedy captures all slots at once, a
    full-length call always takes slot 0): a visit in a slot the kind has not seen captures once more."""
    return key_families(kind) == ("beam",)


def slot_advance(kind):
    """Encoder passes of the call that take the next pipeline slot."""
    return {"batch": 1, "detect": 1, "pipeline": 2, "full": 0, "long": 0}[kind.entry]


# ---- running a kind ---------------------------------------------------------------------------------------------------
class Data:
    """The clips and the audio, read-only."""

    def __init__(self):
        self.mel = scores_model.plain_mels()
        self.mel.setflags(write=False)
        self.audio = lm.pcm()[: SEEK_WINDOWS * lm.WIN - 3000]
        self.audio.setflags(write=False)


def write_model(src_wtw, dst_wtw):
    """full_model's EOT-rich flavour with flatter text rows (gain 10, not 40) and the <|nospeech|> row scaled as
    tests/scores_model.py scales it, by a gain that fits the flatter rows: clips end at different positions, a beam of 2
    and one of 3 part ways, a sample follows its seed, and the timestamp rules force timestamps between the text."""
    from wtw import read_wtw, write_wtw
    full_model.write_eot_rich(src_wtw, dst_wtw, *RICH)
    dims, t = read_wtw(dst_wtw)
    t = {k: np.array(v) for k, v in t.items()}
    t["decoder.token_embedding.weight"][NOSP] *= np.float32(NOSP_GAIN)
    write_wtw(dst_wtw, dims, t)


REFUSED = "refused"
# the getters an entry point defines; the others may hold an earlier call's record
_ALL = ("scores", "token_logprobs", "segments", "segment_scores", "words", "beam_scores", "best_of", "languages",
        "decode_info", "windows")
GETTERS_OF = {
    "full": _ALL, "long": _ALL,
    "batch": ("scores", "token_logprobs", "segments", "segment_scores", "beam_scores", "best_of", "languages",
              "decode_info", "windows"),
    "pipeline": ("scores", "token_logprobs", "best_of", "languages", "decode_info"),
    "detect": (),
}


def _getters(pkg, eng, names, stride):
    def seg_scores():
        n = pkg.lib().wt_last_segment_scores(eng.handle, None, 0)
        if n < 0:
            raise pkg.WtError(-n, "no segment scores")
        return eng.last_segments(with_scores=True)[1]

    table = {
        "scores": eng.last_scores, "token_logprobs": lambda: eng.last_token_logprobs(stride),
        "segments": eng.last_segments, "segment_scores": seg_scores, "words": eng.last_words,
        "beam_scores": eng.last_beam_scores, "best_of": eng.last_best_of, "languages": eng.last_languages,
        "decode_info": eng.last_decode_info, "windows": eng.last_windows,
    }
    out = {}
    for name in names:
        try:
            v = table[name]()
        except pkg.WtError:
            out[name] = REFUSED
            continue
        if isinstance(v, tuple):
            for i, a in enumerate(v):
                out["%s[%d]" % (name, i)] = a
        else:
            out[name] = v
    return out


def _field(a):
    if isinstance(a, (str, bytes)):
        return a
    a = np.ascontiguousarray(a)
    return (a.dtype.str if a.dtype.names is None else str(a.dtype), a.shape, a.itemsize, a.tobytes())


def run(pkg, eng, kind, data):
    """reset, the kind's options, its call: {field: raw bytes (with dtype, shape and item size) or REFUSED}."""
    reset(eng)
    apply(eng, kind.options)
    out = {}
    mel = np.ascontiguousarray(data.mel[list(kind.clips)]) if kind.clips else None
    stride = kind.options.get("max_positions", 31) + 1
    if kind.entry == "batch":
        out["ids"], out["n_ids"] = eng.encdec_tokens_batch(mel)
    elif kind.entry == "detect":
        out["lang"], out["probs"] = eng.detect_language(mel)
    elif kind.entry == "pipeline":
        from conftest import DevBuf
        buf = DevBuf(mel)
        try:
            half, step = len(kind.clips) // 2, (len(kind.clips) // 2) * mel[0].nbytes
            eng.pipeline_submit_dev(buf.data_ptr(), half)
            eng.pipeline_submit_dev(buf.data_ptr() + step, half)
            first, second = eng.pipeline_collect(), eng.pipeline_collect()
        finally:
            buf.free()
        out["ids"] = np.concatenate([first[0], second[0]])
        out["n_ids"] = np.concatenate([first[1], second[1]])
    elif kind.entry == "full":
        out["ids"], out["n_ids"] = eng.encdec_tokens_full(mel)
    elif kind.entry == "long":
        out["text"] = eng.transcribe_long(data.audio).encode()
    else:
        raise ValueError(kind.entry)
    out.update(_getters(pkg, eng, GETTERS_OF[kind.entry], stride))
    return {k: _field(v) for k, v in out.items()}


def first_difference(got, want):
    """None when the two results are equal byte for byte, else (field, index of the first differing element, detail)."""
    for name in sorted(set(got) | set(want)):
        g, w = got.get(name), want.get(name)
        if g == w:
            continue
        if not (isinstance(g, tuple) and isinstance(w, tuple)):
            return name, 0, "%s against %s" % (_brief(g), _brief(w))
        if g[:3] != w[:3]:
            return name, 0, "%s %s against %s %s" % (g[0], g[1], w[0], w[1])
        a, b = np.frombuffer(g[3], np.uint8), np.frombuffer(w[3], np.uint8)
        i = int(np.nonzero(a != b)[0][0]) // g[2]
        return name, i, "%s against %s" % (_element(g, i), _element(w, i))
    return None


def _brief(v):
    return v if isinstance(v, (str, bytes)) or v is None else "%s %s" % (v[0], v[1])


def _element(f, i):
    return f[3][i * f[2]: (i + 1) * f[2]].hex()


def ids_of(result):
    """(ids, n_ids) arrays of a result."""
    f, n = result["ids"], result["n_ids"]
    return np.frombuffer(f[3], np.int64).reshape(f[1]), np.frombuffer(n[3], np.int32)
