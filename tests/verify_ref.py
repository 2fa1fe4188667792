"""CPU reference of gm_verify (test infrastructure; imports nothing of gamesmanmpi_amd).

Given a table (keys, records), the game as ``expand(key) -> (primitive code, children)`` and an
optional overlay ``{key: record, or None to remove the key}``, name every stored position that
the game rules contradict, with its class -- the same rules, in the same order, as
include/gmsolve.h states them for the device:

* bad_primitive: a primitive position whose record is not (primitive value, 0);
* missing_child: an interior position with a child that is not stored;
* bad_value: an interior position whose record is not ``canonical.fold`` of its children's.

Every child's record is read from the table, a primitive child's too.  The device answers a
primitive child from the rules without a lookup (as its backward pass does), so the two agree
on any overlay that touches no primitive position -- and on a clean table.
A removed key is not a stored position: it is not examined, only missed by its parents.
(bad_key and misplaced describe a hash table's keys and slots; no list of (key, record) pairs
can express them.)
"""
import canonical

UNDECIDED = canonical.UNDECIDED
BAD_PRIMITIVE, MISSING_CHILD, BAD_VALUE = "bad_primitive", "missing_child", "bad_value"
CLASSES = ("bad_key", "misplaced", BAD_PRIMITIVE, MISSING_CHILD, BAD_VALUE)
REMOVED = 0xFFFF


def split(rec):
    return int(rec) >> 14, int(rec) & 0x3FFF


class VerifyRef:
    """The table and the game, expanded once; ``offenders(overlay)`` may be asked many times."""

    def __init__(self, keys, records, expand):
        self.table = {int(k): int(r) for k, r in zip(keys, records)}
        self._expand = expand
        self._seen = {}
        self._rev = None

    def expand(self, key):
        e = self._seen.get(key)
        if e is None:
            prim, kids = self._expand(key)[:2]
            e = self._seen[key] = (int(prim), [int(c) for c in kids])
        return e

    def parents(self, key):
        """Stored interior positions with `key` among their children."""
        if self._rev is None:
            self._rev = {}
            for k in self.table:
                for c in set(self.expand(k)[1]):
                    self._rev.setdefault(c, []).append(k)
        return sorted(self._rev.get(key, ()))

    def offenders(self, overlay=None):
        table = dict(self.table)
        for k, r in (overlay or {}).items():
            if r is None or r == REMOVED:
                table.pop(k, None)
            else:
                table[k] = int(r)
        bad = {}
        for k, rec in table.items():
            prim, kids = self.expand(k)
            if prim != UNDECIDED:
                if rec != (prim << 14):
                    bad[k] = BAD_PRIMITIVE
                continue
            pairs = []
            for c in kids:
                if c not in table:
                    pairs = None
                    break
                pairs.append(split(table[c]))
            if pairs is None:
                bad[k] = MISSING_CHILD
            elif split(rec) != canonical.fold(pairs):
                bad[k] = BAD_VALUE
        return bad


def counts(bad):
    """Class counts of an offenders() result, as the fields of gm_verify_t."""
    out = {c: 0 for c in CLASSES}
    for c in bad.values():
        out[c] += 1
    return out


def verify(keys, records, expand, overlay=None):
    return VerifyRef(keys, records, expand).offenders(overlay)
