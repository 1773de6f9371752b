"""TEST INFRASTRUCTURE for the word-level timestamp tests: a writer of a vocab .bin in the
reference layout ([u64 payload][u32 magic][n_mel][n_fft][filters][n_vocab]{u32 len, bytes}) with hand-picked tokens for
the word-splitting rules."""
import string
import struct

import numpy as np

import align_ref

# id -> bytes.  Pieces of multi-byte characters, a token that really is U+FFFD, bytes that never form a character,
# words with and without a leading space, every ASCII punctuation mark and every mark merge_punctuation knows.
_HAND = [
    b" hello", b" world", b"ing", b"s", b"a", b" a ", b" ", b"\n", b" end ", b"x",
    "日".encode()[:2], "日".encode()[2:],                      # 10, 11: a character over two ids
    "本".encode()[:1], "本".encode()[1:2], "本".encode()[2:],  # 12, 13, 14: over three ids
    "\ufffd".encode(),                                              # 15: a genuine U+FFFD
    "\U0001f600".encode()[:2], "\U0001f600".encode()[2:],              # 16, 17: a four-byte character over two ids
    b"\x80", b"\xe6", b"\xff",                                        # 18, 19, 20: never complete
    "語".encode(), " été".encode(), b" (a", b"b)",      # 21 .. 24
]
PUNCT0 = len(_HAND)                                   # one id per ASCII punctuation mark
_HAND += [c.encode() for c in string.punctuation]
PREPEND0 = len(_HAND)                                 # " " + every mark that leads a word
_HAND += [b" " + c.encode() for c in align_ref.PREPEND]
APPEND0 = len(_HAND)                                  # every mark that trails a word
_HAND += [c.encode() for c in align_ref.APPEND]
HAND_TOKENS = list(_HAND)


def write_vocab(path, tokens=HAND_TOKENS, n_mel=80, n_fft=201):
    payload = struct.pack("<Iii", 0x5553454E, n_mel, n_fft) + np.zeros(n_mel * n_fft, np.float32).tobytes()
    payload += struct.pack("<i", len(tokens))
    for t in tokens:
        assert 0 < len(t) <= 255 and b"\0" not in t
        payload += struct.pack("<I", len(t)) + t
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(payload)) + payload)
