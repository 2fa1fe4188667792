"""ctypes view of the 8x8 Othello oracle in oracle/_build/liboracle.so (oracle/othello8.c).

TEST INFRASTRUCTURE ONLY, like oracle/canonical.py.  Positions are the three ABI key words of
include/gmsolve.h (tests/golden/othello8_words.py).
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_P = ctypes.POINTER


class Othello8Oracle:
    def __init__(self):
        # make is a no-op when the library is newer than both sources
        subprocess.check_call(["make", "-s", "-C", HERE])
        L = ctypes.CDLL(os.path.join(HERE, "_build", "liboracle.so"))
        L.oracle_othello8_last_error.restype = ctypes.c_char_p
        L.oracle_othello8_expand.argtypes = [_P(ctypes.c_uint64), _P(ctypes.c_uint64), _P(ctypes.c_int),
                                             _P(ctypes.c_int), _P(ctypes.c_int64)]
        L.oracle_othello8_solve.argtypes = [_P(ctypes.c_uint64), ctypes.c_int, _P(ctypes.c_uint64),
                                            _P(ctypes.c_uint64), ctypes.c_int, _P(ctypes.c_int),
                                            _P(ctypes.c_uint16), _P(ctypes.c_uint64), _P(ctypes.c_uint64),
                                            ctypes.c_uint64, _P(_P(ctypes.c_uint64)), _P(_P(ctypes.c_uint16)),
                                            _P(ctypes.c_uint64)]
        L.oracle_othello8_free.argtypes = [ctypes.c_void_p]
        self.L = L
        self._kids = (ctypes.c_uint64 * (64 * 3))()

    def _fail(self):
        raise RuntimeError(self.L.oracle_othello8_last_error().decode())

    def expand(self, words):
        """(w0, w1, w2) -> (primitive, tier, [child words ...] in gen_moves order)."""
        w = (ctypes.c_uint64 * 3)(*[int(x) for x in words])
        n, p, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        if self.L.oracle_othello8_expand(w, self._kids, ctypes.byref(n), ctypes.byref(p), ctypes.byref(t)) != 0:
            self._fail()
        k = self._kids
        return p.value, t.value, [(k[3 * i], k[3 * i + 1], k[3 * i + 2]) for i in range(n.value)]

    def solve(self, root_words, threads=0, want=0):
        """Strong solve from a root.  Returns a dict: positions, per_tier (index = tier - the
        root's), root_record, word_digest, digest (gm_digest form); with want > 0 also words
        (m, 3) and records (m) of the table in key order -- all entries when want >= positions,
        else `want` evenly spaced ones."""
        w = (ctypes.c_uint64 * 3)(*[int(x) for x in root_words])
        n, wd, gd, nout = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        rr, nt = ctypes.c_uint16(), ctypes.c_int()
        tiers = (ctypes.c_uint64 * 196)()
        kp, rp = _P(ctypes.c_uint64)(), _P(ctypes.c_uint16)()
        if self.L.oracle_othello8_solve(w, threads, ctypes.byref(n), tiers, 196, ctypes.byref(nt), ctypes.byref(rr),
                                        ctypes.byref(wd), ctypes.byref(gd), ctypes.c_uint64(want),
                                        ctypes.byref(kp), ctypes.byref(rp), ctypes.byref(nout)) != 0:
            self._fail()
        out = {"positions": n.value, "per_tier": [int(x) for x in tiers[:nt.value]], "root_record": rr.value,
               "word_digest": wd.value, "digest": gd.value}
        if want:
            m = nout.value
            out["words"] = np.ctypeslib.as_array(kp, (m, 3)).copy()
            out["records"] = np.ctypeslib.as_array(rp, (m,)).copy()
            self.L.oracle_othello8_free(kp)
            self.L.oracle_othello8_free(rp)
        return out
