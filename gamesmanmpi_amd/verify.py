"""The report of ``--verify`` (solver_launcher.py, solve_local.py): gm_verify's counts as one
line, then the offending positions with their moves.

    Verified N positions: consistent
    Verified N positions: K inconsistent (bad_key a, misplaced b, bad_primitive c, missing_child d, bad_value e)

A table that passes is the solution of the game the descriptor (or the explicit graph) states:
the root is stored, every primitive position carries its primitive value, every interior
position the reduction of its children's records.  See DESIGN.md §4.6.
"""
from . import _lib
from .src_utils import to_str

CLASSES = _lib.Verify.CLASSES
SHOWN = 16   # offending positions printed


def consistent(res):
    return res["n_bad"] == 0 and res["root_ok"] == 1


def summary_line(res):
    if consistent(res):
        return "Verified %d positions: consistent" % res["checked"]
    parts = ", ".join("%s %d" % (c, res[c]) for c in CLASSES)
    if not res["root_ok"]:
        parts += ", root record mismatch"
    return "Verified %d positions: %d inconsistent (%s)" % (res["checked"], res["n_bad"], parts)


def _record_text(value, remoteness):
    if value == 3:   # DRAW: no end to count moves to
        return to_str(value)
    return "not stored" if value is None else "%s in %d" % (to_str(value), remoteness)


def offender_lines(solver, keys):
    """One line per offending key and one per child of it, from Solver.moves / Context.moves."""
    from .solver import split_record
    lines = []
    for k in keys[:SHOWN]:
        rec = solver.ctx.query([k])[0]
        lines.append("  %s: %s" % (_show(solver, k), _record_text(*split_record(rec))))
        try:
            kids, recs, best = solver.ctx.moves(k)
        except _lib.GMError:   # a graph context has no descriptor to expand with
            kids, recs, best = _graph_moves(solver, k)
        for i, (c, r) in enumerate(zip(kids, recs)):
            lines.append("    %s %s: %s" % ("*" if i == best else "-", _show(solver, c), _record_text(*split_record(r))))
    return lines


def _graph_moves(solver, key):
    from .solver import best_move
    c = solver.codec
    if not hasattr(c, "off"):
        return [], [], None
    kids = [int(x) for x in c.kids[int(c.off[key]):int(c.off[key + 1])]]
    recs = solver.ctx.query(kids) if kids else []
    return kids, recs, best_move(recs)[0]


def _show(solver, key):
    try:
        return "%r" % (solver.codec.pos(key),)
    except Exception:
        return "key 0x%x" % key


def report(solver, out, statsdir=None):
    """Run gm_verify on the solver's context, write the report to `out` (and verify.json under
    statsdir); True when the table is consistent."""
    import json
    import os
    res, keys = solver.verify(cap=SHOWN)
    out.write(summary_line(res) + "\n")
    if not consistent(res):
        for ln in offender_lines(solver, keys):
            out.write(ln + "\n")
    out.flush()
    if statsdir:
        path = os.path.join(statsdir, "stats", "verify.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(res, consistent=consistent(res), offenders=[hex(k) for k in keys]), f, indent=1)
            f.write("\n")
    return consistent(res)
