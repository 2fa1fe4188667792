"""The layout-independent side of the 8x8 Othello fixtures: ABI key words, tier and the fold
behind ``word_digest`` (othello_8x8_reference.json, oracle_digests.json othello_8x8_*).

A position of the reference plugin at its default 8x8 board is an 18-byte string (white plane,
black plane, turn byte, pass byte; othello_bit_new.py:36-55).  Read as one big-endian integer I
it is the ABI key of include/gmsolve.h, in three little-endian u64 words:

    w0 = I & (2^64 - 1)      w1 = (I >> 64) & (2^64 - 1)      w2 = I >> 128

``word_digest`` of a table is the wrapping sum over its positions of the gm_digest term
(conftest.digest) applied to ONE word per position,

    fold(w0, w1, w2) = mix64(w0 ^ mix64(w1 ^ mix64(w2 ^ FOLD_C)))

so any side computes it without knowing the device's 128-bit key: Python from the string, the
C oracle (oracle/othello8.c, which states the same formula) from its planes, a test from the
words gm_export_key returns.  Nothing here depends on csrc/games.hpp.
"""
import numpy as np

MASK = (1 << 64) - 1
FOLD_C = 0x6A09E667F3BCC908


def words_of(pos):
    """Position string -> (w0, w1, w2)."""
    v = int.from_bytes(pos.encode("ISO-8859-1"), "big")
    return v & MASK, (v >> 64) & MASK, v >> 128


def pos_of(w):
    """(w0, w1, w2) -> position string."""
    v = int(w[0]) | (int(w[1]) << 64) | (int(w[2]) << 128)
    return v.to_bytes(18, "big").decode("ISO-8859-1")


def words_array(positions):
    """Iterable of position strings -> (n, 3) uint64 array."""
    raw = np.frombuffer(b"".join(p.encode("ISO-8859-1") for p in positions), dtype=np.uint8).reshape(-1, 18)
    return bytes_to_words(raw)


def bytes_to_words(raw):
    """(n, 18) uint8 array of position strings -> (n, 3) uint64 array."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    out = np.empty((len(raw), 3), dtype=np.uint64)
    out[:, 2] = raw[:, 0:2].copy().view(">u2")[:, 0]
    out[:, 1] = raw[:, 2:10].copy().view(">u8")[:, 0]
    out[:, 0] = raw[:, 10:18].copy().view(">u8")[:, 0]
    return out


def words_to_bytes(words):
    """(n, 3) uint64 array -> (n, 18) uint8 array of position strings."""
    words = np.asarray(words, dtype=np.uint64)
    out = np.empty((len(words), 18), dtype=np.uint8)
    out[:, 0:2] = words[:, 2].astype(">u2").reshape(-1, 1).view(np.uint8)
    out[:, 2:10] = words[:, 1].astype(">u8").reshape(-1, 1).view(np.uint8)
    out[:, 10:18] = words[:, 0].astype(">u8").reshape(-1, 1).view(np.uint8)
    return out


def _mix64(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xff51afd7ed558ccd)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> np.uint64(33))


def fold(words):
    """(n, 3) uint64 array -> the n folded words."""
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        return _mix64(w[:, 0] ^ _mix64(w[:, 1] ^ _mix64(w[:, 2] ^ np.uint64(FOLD_C))))


def tiers(words):
    """3 * discs + pass count per position (DescOthello8::tier), from the words alone."""
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 3)
    white = (w[:, 1] >> np.uint64(16)) | (w[:, 2] << np.uint64(48))
    black = (w[:, 0] >> np.uint64(16)) | (w[:, 1] << np.uint64(48))
    occ = np.ascontiguousarray(white | black)
    discs = np.unpackbits(occ.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)
    return 3 * discs + (w[:, 0] & np.uint64(0xFF)).astype(np.int64)
