"""Host time of the byte-table readers that csrc/byte_tables.hpp shares: gm_digest of the full
2^32 table on the box engine (one warm-up, then five timed calls, stream idle) and gm_query of
10^5 region keys on dist_sub with 4 virtual ranks (root 0x33557777).  One JSON line.

    python tools/byte_tables_timing.py
    GM_LIB_PATH=<another build of libgmsolve.so> python tools/byte_tables_timing.py

(profiles/byte_tables/)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gamesmanmpi_amd import Context, _lib  # noqa: E402

out = {"lib": os.environ.get("GM_LIB_PATH", "tree")}
ctx = Context(_lib.GAME_SUBTRACT, (8,), device=0)
ctx.solve(0xFFFFFFFF)
ms = []
for i in range(6):
    t0 = time.perf_counter()
    d = ctx.digest()
    ms.append((time.perf_counter() - t0) * 1e3)
out["box_digest"] = [hex(d[0]), d[1]]
out["box_digest_ms"] = ms[1:]
out["box_digest_median_ms"] = float(np.median(ms[1:]))
out["box_digest_spread_ms"] = max(ms[1:]) - min(ms[1:])
ctx.close()

root = 0x33557777
ctx = Context(_lib.GAME_SUBTRACT, (8,), device=0)
ctx.set_option(_lib.OPT_SUB_INTERLEAVE, 10)
ctx.set_option(_lib.OPT_VIRTUAL_RANKS, 4)
ctx.solve(root)
rng = np.random.default_rng(1)
keys = np.zeros(100000, dtype=np.uint64)
for j in range(8):
    keys |= rng.integers(0, ((root >> (4 * j)) & 15) + 1, size=len(keys)).astype(np.uint64) << np.uint64(4 * j)
qms = []
for i in range(3):
    t0 = time.perf_counter()
    r = ctx.query(keys)
    qms.append((time.perf_counter() - t0) * 1e3)
out["dist_sub_query_1e5_ms"] = qms
out["dist_sub_query_sum"] = int(r.astype(np.uint64).sum())
ctx.close()
print(json.dumps(out))
