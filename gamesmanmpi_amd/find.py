"""Which positions of a solved table have a given value and remoteness (``--find``).

A spec is ``VALUE[,VALUE...][:R | :LO-HI | :max]``: values ``win``, ``loss`` (also ``lose``),
``tie``, ``draw`` in any letter case; ``:R`` one remoteness, ``:LO-HI`` an inclusive range,
``:max`` (one value only) the largest remoteness that value has, from the histogram; no suffix
means any remoteness.  ``Context.select()`` / ``Solver.find()`` select on the device (gm_select);
``from_records`` is the numpy reference over (keys, u16 records).

    Found N positions: SPEC
      <repr of position>: WIN in 5

See DESIGN.md §4.9.
"""
from collections import namedtuple

import numpy as np

from . import _lib

NAMES = ("win", "loss", "tie", "draw")                     # by value code
_VALUE = {"win": 0, "loss": 1, "lose": 1, "tie": 2, "draw": 3}
ANY = _lib.SEL_ANY_REM

# values: an OR of _lib.SEL_* (1 << value code); rem_lo..rem_hi inclusive (rem_hi == ANY: no upper
# bound); want_max: ":max", not resolved yet (rem_lo / rem_hi then mean nothing)
Spec = namedtuple("Spec", "values rem_lo rem_hi want_max")


def _remoteness(text, spec):
    if not text.isdigit():
        raise ValueError("spec %r: %r is not a remoteness" % (spec, text))
    r = int(text)
    if r > ANY:
        raise ValueError("spec %r: remoteness %d exceeds %d" % (spec, r, ANY))
    return r


def parse_spec(text):
    """``VALUE[,VALUE...][:R | :LO-HI | :max]`` -> Spec; ValueError names the fault."""
    if not isinstance(text, str) or not text.strip():
        raise ValueError("empty spec")
    head, sep, tail = text.strip().partition(":")
    values = 0
    for name in head.split(","):
        v = _VALUE.get(name.strip().lower())
        if v is None:
            raise ValueError("spec %r: unknown value %r (win, loss, tie, draw)" % (text, name.strip()))
        values |= 1 << v
    if not sep:
        return Spec(values, 0, ANY, False)
    tail = tail.strip().lower()
    if tail == "max":
        if values & (values - 1):
            raise ValueError("spec %r: ':max' needs exactly one value" % text)
        return Spec(values, 0, ANY, True)
    lo, dash, hi = tail.partition("-")
    lo = _remoteness(lo.strip(), text)
    hi = _remoteness(hi.strip(), text) if dash else lo
    if lo > hi:
        raise ValueError("spec %r: the range %d-%d is empty" % (text, lo, hi))
    return Spec(values, lo, hi, False)


def as_spec(spec):
    return spec if isinstance(spec, Spec) else parse_spec(spec)


def resolve(spec, hist):
    """``:max`` replaced by the largest remoteness the spec's value has in the (3, n_rem)
    histogram `hist`; a value without positions (and DRAW, whose record has remoteness 0) gives 0."""
    spec = as_spec(spec)
    if not spec.want_max:
        return spec
    v = spec.values.bit_length() - 1
    r = 0
    if v < 3:
        used = np.nonzero(np.asarray(hist).reshape(3, -1)[v])[0]
        r = int(used[-1]) if len(used) else 0
    return Spec(spec.values, r, r, False)


def spec_text(spec):
    """The normalised text of a spec: ``win,tie:0-2``, ``loss:12``, ``tie:max``, ``draw``."""
    spec = as_spec(spec)
    head = ",".join(NAMES[v] for v in range(4) if (spec.values >> v) & 1)
    if spec.want_max:
        return head + ":max"
    if spec.rem_lo == 0 and spec.rem_hi >= ANY:
        return head
    if spec.rem_lo == spec.rem_hi:
        return "%s:%d" % (head, spec.rem_lo)
    return "%s:%d-%d" % (head, spec.rem_lo, spec.rem_hi)


def match(records, spec):
    """Boolean mask of the u16 records a resolved spec selects (0xFFFF never matches)."""
    spec = as_spec(spec)
    if spec.want_max:
        raise ValueError("resolve ':max' first")
    rec = np.asarray(records, dtype=np.uint16)
    val, rem = (rec >> 14).astype(np.uint32), (rec & 0x3FFF).astype(np.uint32)
    wanted = ((np.uint32(spec.values) >> val) & 1).astype(bool)
    return wanted & (rec != _lib.REC_UNSOLVED) & (rem >= spec.rem_lo) & (rem <= spec.rem_hi)


def from_records(keys, records, spec):
    """The numpy reference of gm_select: (matching keys ascending, their records).  keys: a 1-D
    uint64 array, or (n, words) u64 words least significant first."""
    keys = np.asarray(keys, dtype=np.uint64)
    rec = np.asarray(records, dtype=np.uint16).ravel()
    keep = match(rec, spec)
    keys, rec = keys[keep], rec[keep]
    order = np.argsort(keys, kind="stable") if keys.ndim == 1 else np.lexsort(keys.T)
    return keys[order], rec[order]


def format_lines(n, rows, spec):
    """The block of one spec: the count, then one line per row (position, value, remoteness)."""
    from .verify import _record_text
    lines = ["Found %d positions: %s" % (n, spec_text(spec))]
    for pos, value, remoteness in rows:
        lines.append("  %r: %s" % (pos, _record_text(value, remoteness)))
    return lines


def report(solver, specs, cap, out, statsdir=None, rank=0, world=1, sharded=False, moves=False):
    """--find: per spec, the count and up to `cap` positions ascending by key, written by rank 0
    (and to DIR/stats/find.json with -sd DIR).  Sharded ranks each select among their own keys;
    the counts are summed and the rows merged over the process group, and ``:max`` is resolved
    from the histogram summed over the ranks.  With `moves` every row is followed by the moves
    of its position, indented two more spaces; the moves of all rows of all specs come from one
    Solver.annotate call (not for a solve sharded over processes: no rank holds the table)."""
    import json
    import os
    from .solver import split_record
    specs = [as_spec(s) for s in specs]
    gather = sharded and world > 1
    if gather:
        import torch.distributed as tdist
    hist = None
    if any(s.want_max for s in specs):
        hist = solver.analysis()
        if gather:
            from . import analysis
            parts = [None] * world
            tdist.all_gather_object(parts, hist)
            depth = max(p.shape[1] for p in parts)
            hist = sum(analysis.pad(p, depth) for p in parts)
    found = []
    for spec in specs:
        spec = resolve(spec, hist)
        if gather:
            n, keys, recs = solver.ctx.select(spec.values, spec.rem_lo, spec.rem_hi, cap)
            parts = [None] * world
            tdist.all_gather_object(parts, (n, keys, [int(r) for r in recs]))
            n = sum(p[0] for p in parts)
            merged = sorted((k, r) for p in parts for k, r in zip(p[1], p[2]))[:cap]
            rows = [(solver.codec.pos(k),) + split_record(r) for k, r in merged]
            keys = [k for k, _ in merged]
        else:
            n, rows, keys = solver.find(spec, cap=cap, with_keys=True)
        found.append((spec, n, rows, keys))
    if rank != 0:
        return
    if moves and not gather:
        from .moves import format_rows
        notes = iter(solver.annotate([row[0] for _, _, rows, _ in found for row in rows]))
    for spec, n, rows, _ in found:
        lines = format_lines(n, rows, spec)
        out.write(lines[0] + "\n")
        for ln in lines[1:]:
            out.write(ln + "\n")
            if moves and not gather:
                for mv in format_rows(next(notes)[0], indent="    "):
                    out.write(mv + "\n")
    out.flush()
    if statsdir:
        path = os.path.join(statsdir, "stats", "find.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump([{"spec": spec_text(spec), "n": int(n), "keys": [hex(k) for k in keys],
                        "records": [(int(v) << 14 | int(r)) for _, v, r in rows]}
                       for spec, n, rows, keys in found], f, indent=1)
            f.write("\n")
