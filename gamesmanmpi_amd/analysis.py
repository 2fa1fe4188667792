"""Value-by-remoteness analysis of a solved table.

A histogram is a ``np.uint64`` array of shape ``(3, n_rem)``: rows WIN, LOSS, TIE (the
codes of src/utils.py:4), column r = positions of remoteness r, ``n_rem`` = 1 + the largest
remoteness.  ``Context.histogram()`` / ``Solver.analysis()`` count it on the device
(gm_histogram); ``from_records`` is the numpy reference over u16 records.
"""
import numpy as np

from . import _lib

VALUES = ("win", "loss", "tie")
CHUNK = 1 << 24   # records per bincount call (bounds the temporaries of a 2^28-record table)
HEADER = ("Remoteness", "Win", "Lose", "Tie", "Total")


def from_records(records, weights=None):
    """The histogram of u16 records ((value << 14) | remoteness; 0xFFFF entries are skipped).
    ``weights``: positions each record stands for (an orbit size), default 1."""
    rec = np.asarray(records, dtype=np.uint16).ravel()
    w = None if weights is None else np.asarray(weights, dtype=np.uint64).ravel()
    if w is not None and len(w) != len(rec):
        raise ValueError("weights and records differ in length")
    keep = rec != _lib.REC_UNSOLVED
    rec = rec[keep]
    if w is not None:
        w = w[keep]
    flat = np.zeros(1 << 16, dtype=np.uint64)   # one bin per u16 record
    if w is None:
        for a in range(0, len(rec), CHUNK):
            flat += np.bincount(rec[a:a + CHUNK], minlength=1 << 16).astype(np.uint64)
    else:
        np.add.at(flat, rec, w)
    if flat[3 << 14:].any():
        raise ValueError("a record holds a value other than WIN, LOSS, TIE")
    return trim(flat[:3 << 14].reshape(3, 1 << 14))


def pad(hist, n_rem):
    """``hist`` widened with zero columns to ``n_rem`` (sums of arrays of different depth)."""
    hist = np.asarray(hist, dtype=np.uint64).reshape(3, -1)
    out = np.zeros((3, max(n_rem, hist.shape[1])), dtype=np.uint64)
    out[:, :hist.shape[1]] = hist
    return out


def trim(hist):
    """``hist`` without its trailing all-zero columns."""
    hist = np.asarray(hist, dtype=np.uint64).reshape(3, -1)
    used = np.nonzero(hist.sum(axis=0))[0]
    return hist[:, :int(used[-1]) + 1 if len(used) else 0]


def summarize(hist):
    """Totals per value, the position total and the largest remoteness per value (None for a
    value no position has)."""
    hist = np.asarray(hist, dtype=np.uint64).reshape(3, -1)
    out = {"positions": int(hist.sum()), "n_remoteness": int(hist.shape[1])}
    for v, name in enumerate(VALUES):
        used = np.nonzero(hist[v])[0]
        out[name] = int(hist[v].sum())
        out["max_remoteness_" + name] = int(used[-1]) if len(used) else None
    return out


def format_table(hist):
    """Fixed-width text: the header, one row per remoteness (all-zero rows too, so the rows
    are positional) and a Total row."""
    hist = np.asarray(hist, dtype=np.uint64).reshape(3, -1)
    rows = [[str(r)] + [str(int(hist[v, r])) for v in range(3)] + [str(int(hist[:, r].sum()))]
            for r in range(hist.shape[1])]
    rows.append(["Total"] + [str(int(hist[v].sum())) for v in range(3)] + [str(int(hist.sum()))])
    width = [max(len(HEADER[i]), max(len(row[i]) for row in rows)) for i in range(5)]
    lines = ["  ".join(cell.rjust(width[i]) for i, cell in enumerate(row)) for row in [list(HEADER)] + rows]
    return "\n".join(lines)


def parse_table(text):
    """The histogram ``format_table`` printed (the Total row is checked, not returned)."""
    lines = [ln.split() for ln in text.strip().splitlines()]
    if not lines or tuple(lines[0]) != HEADER or lines[-1][0] != "Total":
        raise ValueError("not an analysis table")
    body = lines[1:-1]
    hist = np.zeros((3, len(body)), dtype=np.uint64)
    for r, row in enumerate(body):
        if int(row[0]) != r:
            raise ValueError("row %d is labelled %s" % (r, row[0]))
        hist[:, r] = [int(x) for x in row[1:4]]
        if int(row[4]) != int(hist[:, r].sum()):
            raise ValueError("row %d does not add up" % r)
    if [int(x) for x in lines[-1][1:]] != [int(hist[v].sum()) for v in range(3)] + [int(hist.sum())]:
        raise ValueError("the Total row does not add up")
    return hist


def as_json(hist):
    """``summarize`` plus the three rows as lists (stats/analysis.json)."""
    hist = np.asarray(hist, dtype=np.uint64).reshape(3, -1)
    out = summarize(hist)
    for v, name in enumerate(VALUES):
        out[name + "_by_remoteness"] = [int(x) for x in hist[v]]
    return out
