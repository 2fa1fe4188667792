"""The record / preference-score algebra of csrc/gm_common.hpp, checked exhaustively on the host.

Every engine decides a position as parent_score(max of its children's scores); that must be
exactly the (value, remoteness) rule of oracle/canonical.py: fold.  The functions are compiled
from the header itself (tests/csrc/score_shim.cpp) with the host C++ compiler and compared, over
every value and every 14-bit remoteness, with fold and with plain record arithmetic.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

from canonical import LOSS, TIE, WIN, fold

RMAX = 0x3FFF
CLASSES = (WIN, LOSS, TIE)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("score_shim") / "libscore_shim.so")
    src = os.path.join(REPO, "tests", "csrc", "score_shim.cpp")
    flags = ["-O1", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(REPO, "gamesmanmpi_amd", "csrc"), src, "-o", out]
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx:
        cmd = [cxx] + flags
    else:   # host-only compile with the HIP compiler driver
        hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
        cmd = [hipcc, "-x", "c++"] + flags
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "%s\n%s%s" % (" ".join(cmd), r.stdout, r.stderr)
    return Shim(ctypes.CDLL(out))


class Shim:
    def __init__(self, lib):
        self.lib = lib

    def _call(self, name, x, in_dtype, out_dtype):
        x = np.ascontiguousarray(np.atleast_1d(x), dtype=in_dtype)
        out = np.empty(len(x), dtype=out_dtype)
        f = getattr(self.lib, "shim_" + name)
        f.restype = None
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        f(x.ctypes.data, out.ctypes.data, len(x))
        return out

    def score_of_primitive(self, v):
        return self._call("score_of_primitive", v, np.int32, np.uint16)

    def parent_score(self, b):
        return self._call("parent_score", b, np.uint32, np.uint16)

    def record_of_score(self, s):
        return self._call("record_of_score", s, np.uint16, np.uint16)

    def score_of_record(self, r):
        return self._call("score_of_record", r, np.uint16, np.uint16)

    def score_overflows(self, b):
        return self._call("score_overflows", b, np.uint32, np.uint8).astype(bool)

    def parent_code(self, b):
        return self._call("parent_code", b, np.uint32, np.uint32)

    def record_of_code(self, b):
        return self._call("record_of_code", b, np.uint8, np.uint16)


def records(v, rems=None):
    """Every record of value v (or those of the remotenesses given)."""
    rems = np.arange(RMAX + 1) if rems is None else np.asarray(rems)
    return ((v << 14) | rems).astype(np.uint16)


def packed(value_rem):
    return (value_rem[0] << 14) | value_rem[1]


ALL = np.concatenate([records(v) for v in CLASSES])   # 49,152 records


def test_round_trip(shim):
    s = shim.score_of_record(ALL)
    assert np.all(s != 0)
    assert len(np.unique(s)) == len(ALL)
    assert np.array_equal(shim.record_of_score(s), ALL)
    assert shim.score_of_record(0xFFFF)[0] == 0
    assert shim.record_of_score(0)[0] == 0xFFFF
    # the score classes: nothing but 0 maps to "unsolved", and every score of a class round-trips
    every = np.arange(1 << 16, dtype=np.uint16)
    back = shim.record_of_score(every)
    assert np.array_equal(back == 0xFFFF, every < 0x4000)
    assert np.array_equal(shim.score_of_record(back[0x4000:]), every[0x4000:])


def test_primitives(shim):
    for v in CLASSES:
        assert shim.score_of_primitive(v)[0] == shim.score_of_record(v << 14)[0]


def test_order_is_the_preference_order_of_fold(shim):
    s = shim.score_of_record(ALL).astype(np.int64)
    by_score = ALL[np.argsort(-s, kind="stable")]
    want = np.concatenate([records(LOSS), records(TIE), records(WIN)[::-1]])
    assert np.array_equal(by_score, want)


@pytest.mark.parametrize("v", CLASSES)
def test_single_child(shim, v):
    rems = np.arange(0x3FFD + 1)
    got = shim.record_of_score(shim.parent_score(shim.score_of_record(records(v, rems))))
    want = np.array([packed(fold([(v, int(r))])) for r in rems], dtype=np.uint16)
    assert np.array_equal(got, want)


def test_overflow(shim):
    for v in CLASSES:
        over = shim.score_overflows(shim.score_of_record(records(v)))
        assert not over[:0x3FFE].any(), (v, np.flatnonzero(over[:0x3FFE]))
        assert over[0x3FFF], v   # the parent's remoteness would be 0x4000
        if not over[0x3FFE]:     # allowed through: then the parent's record must be the true one
            got = shim.record_of_score(shim.parent_score(shim.score_of_record(records(v, [0x3FFE]))))
            assert got[0] == packed(fold([(v, 0x3FFE)]))


def draw_multisets(n, max_children, max_rem, classes, seed):
    """n multisets of 1..max_children (value, remoteness) children as (values, rems, count)
    arrays, rows padded.  A multiset draws its values from a random non-empty subset of
    `classes`, its remotenesses from the whole range or from a window of 4 around a random
    centre (so equal and adjacent remotenesses compete), or the ends of the range."""
    rng = np.random.default_rng(seed)
    count = rng.integers(1, max_children + 1, size=n)
    subset = rng.integers(1, 1 << len(classes), size=n)
    allowed = np.zeros((1 << len(classes), len(classes)), dtype=np.int64)
    for bits in range(1, 1 << len(classes)):
        mine = [c for j, c in enumerate(classes) if bits >> j & 1]
        allowed[bits, :len(mine)] = mine
    size = np.array([bin(b).count("1") for b in range(1 << len(classes))])[subset]
    pick = (rng.random((n, max_children)) * size[:, None]).astype(np.int64)
    values = allowed[subset[:, None], pick]
    wide = rng.integers(0, max_rem + 1, size=(n, max_children))
    centre = rng.integers(0, max_rem + 1, size=(n, 1))
    near = np.clip(centre + rng.integers(-2, 3, size=(n, max_children)), 0, max_rem)
    ends = np.where(rng.random((n, max_children)) < 0.5, rng.integers(0, 3, size=(n, max_children)),
                    max_rem - rng.integers(0, 3, size=(n, max_children)))
    how = rng.integers(0, 3, size=(n, 1))
    rems = np.where(how == 0, wide, np.where(how == 1, near, ends))
    return values, rems, count


def class_sets(values, count, classes):
    """Per multiset, the bit set of the classes among its children."""
    live = np.arange(values.shape[1])[None, :] < count[:, None]
    bits = np.zeros(len(values), dtype=np.int64)
    for j, c in enumerate(classes):
        bits |= ((values == c) & live).any(axis=1).astype(np.int64) << j
    return bits


def test_multisets(shim):
    n, width = 100_000, 16
    values, rems, count = draw_multisets(n, width, 0x3FFD, CLASSES, seed=20240611)
    assert count.min() == 1 and count.max() == width
    bits = class_sets(values, count, CLASSES)
    for want in (0b011, 0b101, 0b110, 0b111):   # every class pair, and all three, at one node
        assert np.count_nonzero(bits == want) >= 1000, (want, np.count_nonzero(bits == want))
    live = np.arange(width)[None, :] < count[:, None]
    scores = shim.score_of_record(((values << 14) | rems).astype(np.uint16).ravel()).reshape(n, width)
    best = np.where(live, scores, 0).max(axis=1)
    assert not shim.score_overflows(best).any()
    got = shim.record_of_score(shim.parent_score(best))
    v_l, r_l, c_l = values.tolist(), rems.tolist(), count.tolist()
    want = np.array([packed(fold(zip(v_l[i][:c_l[i]], r_l[i][:c_l[i]]))) for i in range(n)], dtype=np.uint16)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), [(v_l[i][:c_l[i]], r_l[i][:c_l[i]], hex(got[i]), hex(want[i])) for i in bad[:3]])


def test_byte_codes(shim):
    rems = np.arange(127)
    assert shim.record_of_code(0)[0] == 0xFFFF
    assert np.array_equal(shim.record_of_code(rems + 1), records(WIN, rems))
    assert np.array_equal(shim.record_of_code(255 - rems), records(LOSS, rems))
    # one child
    for v, code in ((WIN, rems[:126] + 1), (LOSS, 255 - rems[:126])):
        got = shim.record_of_code(shim.parent_code(code).astype(np.uint8))
        assert np.array_equal(got, [packed(fold([(v, int(r))])) for r in rems[:126]])
        assert np.all(shim.parent_code(code) < 256)
    # the codes order like the u16 scores of their records
    codes = np.arange(1, 256)
    s = shim.score_of_record(shim.record_of_code(codes)).astype(np.int64)
    assert np.all(np.diff(s) > 0)
    # multisets of WIN and LOSS children: the parent of the max code is fold's
    n, width = 20_000, 16
    values, rems, count = draw_multisets(n, width, 125, (WIN, LOSS), seed=7)
    assert np.count_nonzero(class_sets(values, count, (WIN, LOSS)) == 0b11) >= 1000
    live = np.arange(width)[None, :] < count[:, None]
    child = np.where(values == WIN, rems + 1, 255 - rems)
    best = np.where(live, child, 0).max(axis=1)
    got = shim.record_of_code(shim.parent_code(best).astype(np.uint8))
    v_l, r_l, c_l = values.tolist(), rems.tolist(), count.tolist()
    want = [packed(fold(zip(v_l[i][:c_l[i]], r_l[i][:c_l[i]]))) for i in range(n)]
    assert np.array_equal(got, want)
