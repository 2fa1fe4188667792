"""Write tests/golden/histograms.json: value-by-remoteness counts of whole solved games.

    python tests/golden/make_histograms.py

subtract_8: the 2^32-position 8-heap game, solved by the repo's C oracle
(oracle_subtract_dense_mt) and counted with chunked np.bincount over its u16 records
(about 8 GB of host memory, under a minute on 8 cores).  Rows are WIN, LOSS, TIE by
remoteness, as gamesmanmpi_amd.analysis.from_records lays them out.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from conftest import Oracle   # noqa: E402

CHUNK = 1 << 26


def dense_histogram(recs):
    flat = np.zeros(1 << 16, dtype=np.int64)
    for a in range(0, len(recs), CHUNK):
        flat += np.bincount(recs[a:a + CHUNK], minlength=1 << 16)
    assert flat[0xFFFF] == 0 and flat[3 << 14:].sum() == 0
    by_value = flat[:3 << 14].reshape(3, 1 << 14)
    n_rem = int(np.nonzero(by_value.sum(axis=0))[0][-1]) + 1
    return by_value[:, :n_rem]


def main():
    h = dense_histogram(Oracle().subtract_dense_mt(8))
    out = {"subtract_8": {"n_rem": int(h.shape[1]), "positions": int(h.sum()),
                          "win": [int(x) for x in h[0]], "loss": [int(x) for x in h[1]],
                          "tie": [int(x) for x in h[2]]}}
    with open(os.path.join(HERE, "histograms.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print({k: (v["n_rem"], v["positions"]) for k, v in out.items()})


if __name__ == "__main__":
    main()
