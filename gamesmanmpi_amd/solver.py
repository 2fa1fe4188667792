"""Host-side solver API: the drop-in for the reference's Process/Job engine.

``Solver(module)`` plays the role of ``Process`` + ``GameState``
(reference src/new_process.py:62-94, src/game_state.py): it binds a plugin
module to a device descriptor, solves every position reachable from the root
in one ``gm_solve`` call, and answers lookups (the reference's
``resolved``/``remote`` tables, src/new_process.py:76-78).
"""
import ctypes
import os

import numpy as np

from . import _lib, games
from .src_utils import to_str

WIN, LOSS, TIE, DRAW, UNDECIDED = 0, 1, 2, 3, 4


def split_record(rec):
    """u16 record -> (value, remoteness); (None, None) for 0xFFFF."""
    rec = int(rec)
    if rec == _lib.REC_UNSOLVED:
        return None, None
    return rec >> 14, rec & 0x3FFF


def score_of_record(rec):
    """The preference score of a child's record (csrc/gm_common.hpp): the mover prefers the
    child with the largest -- a LOSS child over a TIE child over a WIN child, the shortest
    LOSS or TIE, the longest WIN.  0 for 0xFFFF."""
    rec = int(rec)
    if rec == _lib.REC_UNSOLVED:
        return 0
    v, r = rec >> 14, rec & 0x3FFF
    if v == WIN:
        return 0x4000 | r
    return (0x8000 if v == TIE else 0xC000) | (0x3FFF - r)


def move_rank(rec):
    """score_of_record with the DRAW children of a loopy solve in their place: LOSS > TIE >
    DRAW > WIN (csrc/graph_common.hpp loopy_key).  Without a DRAW record the order is
    score_of_record's."""
    return 0xFFFF if int(rec) == _lib.REC_DRAW else 2 * score_of_record(rec)


def best_move(records):
    """Index of the child the solver would play among `records` (the first of equals), and the
    parent's (value, remoteness) that choice gives; (None, None) without children."""
    if not len(records):
        return None, None
    best = max(range(len(records)), key=lambda i: move_rank(records[i]))
    v, r = split_record(records[best])
    if v is None:
        return best, (None, None)
    if v == DRAW:
        return best, (DRAW, 0)
    return best, ({LOSS: WIN, TIE: TIE, WIN: LOSS}[v], r + 1)


class NoDescriptor(RuntimeError):
    pass


class Context:
    """Thin RAII wrapper over one ``gm_ctx``."""

    def __init__(self, game_id, params=(), device=-1):
        self.L = _lib.lib()
        arr = (ctypes.c_int32 * max(1, len(params)))(*params)
        h = ctypes.c_void_p()
        _lib.check(self.L.gm_open(game_id, arr, len(params), device, ctypes.byref(h)))
        self.h = h
        self.game_id = game_id
        self.params = tuple(params)
        # u64 words per key: 1, or 3 for boards past 64 bits (Othello 8x8); keys are then Python
        # ints on the host and (n, words) uint64 arrays in bulk.  Every call goes through the
        # gm_*_key forms, which equal the one-word forms on a one-word game
        self.words = self.L.gm_key_words(h)

    def _words(self, key):
        """One key (a Python int) as the words array the gm_*_key calls take."""
        return (ctypes.c_uint64 * self.words)(*_lib.int_to_words(key, self.words))

    def _keys(self, a):
        """An (n, words) array the library filled, as callers get it: 1-D for one-word keys."""
        return a if self.words > 1 else a[:, 0]

    def set_option(self, opt, value):
        _lib.check(self.L.gm_set_option(self.h, opt, int(value)))

    def set_stream(self, stream_ptr):
        _lib.check(self.L.gm_set_stream(self.h, ctypes.c_void_p(stream_ptr or 0)))

    def set_comm(self, rank, world, uid=None):
        buf = ctypes.create_string_buffer(uid, 128) if uid is not None else None
        _lib.check(self.L.gm_set_comm(self.h, rank, world, buf, 128 if buf is not None else 0))

    def initial(self):
        w = (ctypes.c_uint64 * self.words)()
        _lib.check(self.L.gm_pack_initial_key(self.h, w))
        return _lib.words_to_int(w)

    def solve(self, root):
        n = ctypes.c_uint64()
        r = ctypes.c_uint16()
        _lib.check(self.L.gm_solve_key(self.h, self._words(root), ctypes.byref(n), ctypes.byref(r)))
        return n.value, r.value

    def import_table(self, keys, records, root):
        """gm_import: load (keys, records) as the table of a solve from `root`.  Keys as query()
        takes them, in any order.  Returns (n_positions, root record; 0xFFFF when the root is
        not among the keys)."""
        keys = self.key_array(keys)
        recs = np.ascontiguousarray(records, dtype=np.uint16)
        if len(recs) != len(keys):
            raise ValueError("import_table: %d keys, %d records" % (len(keys), len(recs)))
        n = ctypes.c_uint64()
        r = ctypes.c_uint16()
        _lib.check(self.L.gm_import(self.h, self._words(root), keys.ctypes.data if len(keys) else None,
                                    recs.ctypes.data if len(recs) else None, len(keys), ctypes.byref(n),
                                    ctypes.byref(r)))
        return n.value, r.value

    def key_array(self, keys):
        """Keys (Python ints, or an (n, words) uint64 array) -> the array gm_query_key takes."""
        if self.words == 1:
            return np.ascontiguousarray(keys, dtype=np.uint64)
        a = np.asarray(keys) if not isinstance(keys, list) else None
        if a is not None and a.dtype == np.uint64 and a.ndim == 2:
            return np.ascontiguousarray(a)
        return np.array([_lib.int_to_words(k, self.words) for k in keys], dtype=np.uint64).reshape(-1, self.words)

    def solve_graph(self, prim, off, kids):
        """gm_solve_graph over an explicit graph (gamesmanmpi_amd/graph.py)."""
        import numpy as np
        prim = np.ascontiguousarray(prim, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        kids = np.ascontiguousarray(kids, dtype=np.uint32)
        r = ctypes.c_uint16()
        _lib.check(self.L.gm_solve_graph(self.h, len(prim), prim.ctypes.data, off.ctypes.data,
                                         kids.ctypes.data if len(kids) else None, ctypes.byref(r)))
        return len(prim), r.value

    def export(self):
        """Sorted keys and records (multi-word keys: an (n, words) uint64 array)."""
        n = ctypes.c_uint64()
        _lib.check(self.L.gm_export_key(self.h, None, None, 0, ctypes.byref(n)))
        keys = np.empty((n.value, self.words), dtype=np.uint64)
        recs = np.empty(n.value, dtype=np.uint16)
        _lib.check(self.L.gm_export_key(self.h, keys.ctypes.data, recs.ctypes.data, n.value, ctypes.byref(n)))
        return self._keys(keys[:n.value]), recs[:n.value]

    def query(self, keys):
        keys = self.key_array(keys)
        out = np.empty(len(keys), dtype=np.uint16)
        _lib.check(self.L.gm_query_key(self.h, keys.ctypes.data, out.ctypes.data, len(keys)))
        return out

    def draw_count(self):
        """gm_draw_count: the DRAW positions of the last solve (0 unless it was a loopy graph solve)."""
        n = ctypes.c_uint64()
        _lib.check(self.L.gm_draw_count(self.h, ctypes.byref(n)))
        return n.value

    def digest(self):
        d, n = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self.L.gm_digest(self.h, ctypes.byref(d), ctypes.byref(n)))
        return d.value, n.value

    def histogram(self):
        """gm_histogram: this rank's positions by value and remoteness, a (3, n_rem) uint64
        array with rows WIN, LOSS, TIE (gamesmanmpi_amd/analysis.py)."""
        n_rem, n = ctypes.c_int(), ctypes.c_uint64()
        _lib.check(self.L.gm_histogram(self.h, None, 0, ctypes.byref(n_rem), ctypes.byref(n)))
        out = np.zeros((3, n_rem.value), dtype=np.uint64)
        _lib.check(self.L.gm_histogram(self.h, out.ctypes.data if out.size else None, n_rem.value,
                                       ctypes.byref(n_rem), ctypes.byref(n)))
        return out

    def verify(self, cap=64):
        """gm_verify: the held table checked against the game rules on the device.  Returns
        (dict of gm_verify_t plus n_bad, up to `cap` offending keys as Python ints, ascending)."""
        out = _lib.Verify()
        n_bad = ctypes.c_uint64()
        keys = np.zeros((max(1, cap), self.words), dtype=np.uint64)
        _lib.check(self.L.gm_verify(self.h, ctypes.byref(out), keys.ctypes.data if cap else None, cap,
                                    ctypes.byref(n_bad)))
        n = min(cap, n_bad.value)
        return out.as_dict(), [_lib.words_to_int(keys[i]) for i in range(n)]

    def select(self, values, rem_lo=0, rem_hi=_lib.SEL_ANY_REM, cap=64, as_array=False):
        """gm_select: the held positions whose value is among `values` (an OR of _lib.SEL_*) and
        whose remoteness lies in [rem_lo, rem_hi], found on the device.  Returns (n, keys,
        records): n counts every match, keys are up to `cap` of them ascending -- Python ints, or
        with as_array the array export() returns (1-D uint64, (m, words) for multi-word keys) --
        and records their u16 records."""
        what = _lib.Select(int(values), int(rem_lo), int(rem_hi), 0)
        n = ctypes.c_uint64()
        cap = int(cap)
        keys = np.zeros((max(1, cap), self.words), dtype=np.uint64)
        recs = np.zeros(max(1, cap), dtype=np.uint16)
        _lib.check(self.L.gm_select(self.h, ctypes.byref(what), keys.ctypes.data if cap else None,
                                    recs.ctypes.data if cap else None, cap, ctypes.byref(n)))
        m = min(cap, n.value)
        if as_array:
            return n.value, self._keys(keys[:m]), recs[:m]
        return n.value, [_lib.words_to_int(keys[i]) for i in range(m)], recs[:m]

    def poke(self, key, record):
        """gm_poke (test hook): overwrite one held position's record; 0xFFFF removes it."""
        _lib.check(self.L.gm_poke(self.h, self._words(key), int(record)))

    def expand(self, key):
        """gm_expand_host: (primitive code, children in the plugin's gen_moves order, tier)."""
        n, p, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        kids = (ctypes.c_uint64 * (64 * self.words))()
        _lib.check(self.L.gm_expand_host_key(self.h, self._words(key), kids, 64, ctypes.byref(n), ctypes.byref(p),
                                             ctypes.byref(t)))
        W = self.words
        return p.value, [_lib.words_to_int(kids[W * i:W * i + W]) for i in range(n.value)], t.value

    def moves(self, key):
        """What the mover can do at `key`: (children in the plugin's gen_moves order, their
        records, the index of the child the solver would play); a primitive position has no
        moves and index None."""
        prim, kids, _ = self.expand(key)
        if prim != UNDECIDED or not kids:
            return [], np.zeros(0, dtype=np.uint16), None
        recs = self.query(kids)
        return kids, recs, best_move(recs)[0]

    def moves_batch(self, keys, children=True):
        """gm_moves: every key's record, children and the mover's choice from one device call.
        Keys as query() takes them, in any order, repeats allowed.  Returns (heads, child_keys,
        child_records): heads a structured array (_lib.moves_dtype: first, count, best, record,
        n_best), child_keys of shape (total,) -- (total, words) for multi-word keys -- in key
        order, each key's children in the plugin's gen_moves order, child_records their u16
        records.  children=False: heads only (child_keys and child_records None)."""
        keys = self.key_array(keys)
        n = len(keys)
        heads = np.zeros(n, dtype=_lib.moves_dtype())
        total = ctypes.c_uint64()
        kp = keys.ctypes.data if n else None
        hp = heads.ctypes.data if n else None
        if not children:
            _lib.check(self.L.gm_moves(self.h, kp, n, hp, None, None, 0, ctypes.byref(total)))
            return heads, None, None
        cap = 12 * n + 64   # a guess; a batch with more children is asked again with its total
        while True:
            ck = np.empty((cap, self.words), dtype=np.uint64)
            cr = np.empty(cap, dtype=np.uint16)
            rc = self.L.gm_moves(self.h, kp, n, hp, ck.ctypes.data, cr.ctypes.data, cap, ctypes.byref(total))
            if rc == -8 and total.value > cap:   # GM_E_CAP: heads and the total are set
                cap = total.value
                continue
            _lib.check(rc)
            break
        t = total.value
        return heads, self._keys(ck[:t]), cr[:t]

    def reach(self, starts, mover=_lib.REACH_ALL, other=_lib.REACH_ALL, max_plies=0, cap=0, plies=True):
        """gm_reach: the positions reachable from `starts` (keys as query() takes them) when the
        starts' mover follows policy `mover` and the opponent `other` (_lib.REACH_*), found on
        the device.  Returns (out, ply_counts, keys, records, sides): out the dict of
        gm_reach_out_t, ply_counts a uint64 array with one entry per ply reached (None with
        plies=False), keys up to `cap` reached positions ascending as export() returns them,
        records their u16 records and sides their side bits (bit 0 an even ply, bit 1 an odd
        one).  cap=0: counts only (keys, records and sides None)."""
        keys = self.key_array(starts)
        n = len(keys)
        how = _lib.Reach(int(mover), int(other), int(max_plies), 0)
        out = _lib.ReachOut()
        cap = int(cap)
        kw = np.zeros((max(1, cap), self.words), dtype=np.uint64)
        rr = np.zeros(max(1, cap), dtype=np.uint16)
        ss = np.zeros(max(1, cap), dtype=np.uint8)
        ply_cap = 1024 if plies else 0
        while True:
            pc = np.zeros(max(1, ply_cap), dtype=np.uint64)
            rc = self.L.gm_reach(self.h, ctypes.byref(how), keys.ctypes.data if n else None, n, ctypes.byref(out),
                                 pc.ctypes.data if ply_cap else None, ply_cap, kw.ctypes.data if cap else None,
                                 rr.ctypes.data if cap else None, ss.ctypes.data if cap else None, cap)
            if rc == -8 and out.plies > ply_cap:   # GM_E_CAP: out is set
                ply_cap = out.plies
                continue
            _lib.check(rc)
            break
        pcs = pc[:out.plies].copy() if plies else None
        if not cap:
            return out.as_dict(), pcs, None, None, None
        m = min(cap, out.n)
        return out.as_dict(), pcs, self._keys(kw[:m]), rr[:m], ss[:m]

    def stats(self):
        s = _lib.Stats()
        _lib.check(self.L.gm_stats(self.h, ctypes.byref(s)))
        return s.as_dict()

    def tier_counts(self):
        n = ctypes.c_int()
        _lib.check(self.L.gm_tier_counts(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.uint64)
        _lib.check(self.L.gm_tier_counts(self.h, out.ctypes.data, n.value, ctypes.byref(n)))
        return out[:n.value]

    def rank_stats(self):
        """Per rank of the last split box solve (gm_rank_stats): GPU ms from its first tier launch
        to its last (GM_OPT_TIMING), boxes computed, halo bytes received per solve."""
        n = ctypes.c_int()
        _lib.check(self.L.gm_rank_stats(self.h, None, None, None, 0, ctypes.byref(n)))
        ms = np.zeros(max(1, n.value), dtype=np.float64)
        boxes = np.zeros(max(1, n.value), dtype=np.uint64)
        recv = np.zeros(max(1, n.value), dtype=np.uint64)
        _lib.check(self.L.gm_rank_stats(self.h, ms.ctypes.data, boxes.ctypes.data, recv.ctypes.data, n.value,
                                        ctypes.byref(n)))
        return [{"kernel_ms": float(ms[i]), "boxes": int(boxes[i]), "recv_bytes": int(recv[i])}
                for i in range(n.value)]

    def rank_op_ms(self, rank):
        """GPU ms of every op of `rank`'s op list in the last split box solve (GM_OPT_TIMING)."""
        n = ctypes.c_int()
        _lib.check(self.L.gm_rank_op_ms(self.h, rank, None, 0, ctypes.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.float64)
        _lib.check(self.L.gm_rank_op_ms(self.h, rank, out.ctypes.data, n.value, ctypes.byref(n)))
        return out[:n.value]

    def adopt_dense_table(self, dev_ptr, nbytes):
        _lib.check(self.L.gm_adopt_buffer(self.h, _lib.BUF_DENSE_TABLE, ctypes.c_void_p(dev_ptr), nbytes))

    def dense_table(self):
        p, b = ctypes.c_void_p(), ctypes.c_uint64()
        _lib.check(self.L.gm_dense_table(self.h, ctypes.byref(p), ctypes.byref(b)))
        return p.value, b.value

    def close(self):
        if getattr(self, "h", None):
            self.L.gm_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Solver:
    """Strong-solve a plugin module on the GPU.

    ``module`` is a GamesmanMPI plugin; ``root`` defaults to
    ``module.initial_position()`` (GameState.INITIAL_POS, src/game_state.py:15).
    A plugin that no device descriptor reproduces is solved as an explicit graph
    (gamesmanmpi_amd/graph.py): the host enumerates it with the plugin's own
    functions and the device resolves it; ``graph=True`` forces that path,
    ``graph=False`` raises NoDescriptor instead.  ``loopy=True`` is for games in which a
    position can repeat: it takes the graph path whatever the plugin is and solves with
    GM_OPT_LOOPY, so that cycles are allowed and a position neither side can decide is DRAW.
    """

    def __init__(self, module, root=None, device=-1, engine=None, codec=None, graph=None, loopy=False):
        self.module = module
        self.root = module.initial_position() if root is None else root
        self.loopy = bool(loopy)
        if self.loopy:
            if graph is False or (codec is not None and codec.game_id != _lib.GAME_GRAPH):
                raise ValueError("a loopy solve is an explicit-graph solve")
            graph = True
        if codec is None and not graph:
            codec = games.identify(module, self.root)
        if codec is None:
            if graph is False:
                raise NoDescriptor(
                    "no device descriptor reproduces plugin %r; supported: Four-To-One, "
                    "tic-tac-toe (mttt / numpy), Toot-and-Otto and Othello bitboards, "
                    "the subtraction game" % getattr(module, "__file__", module))
            from .graph import GraphCodec
            codec = GraphCodec(module, self.root)
        self.codec = codec
        self.ctx = Context(self.codec.game_id, self.codec.params, device)
        if engine is not None:
            self.ctx.set_option(_lib.OPT_ENGINE, engine)
        if self.loopy:
            self.ctx.set_option(_lib.OPT_LOOPY, 1)
        self.root_key = self.codec.key(self.root)
        self.n_positions = None
        self.root_record = None

    def solve(self):
        if self.codec.game_id == _lib.GAME_GRAPH:
            c = self.codec
            _, self.root_record = self.ctx.solve_graph(c.prim, c.off, c.kids)
            self.n_positions = c.n_positions   # every orbit member (gamesmanmpi_amd/graph.py)
        else:
            self.n_positions, self.root_record = self.ctx.solve(self.root_key)
        return self.n_positions, self.root_record

    def load(self, keys, records):
        """In place of solve(): load a stored table of this game and root onto the device
        (gm_import).  lookup(), table(), analysis(), verify() and moves() then answer for it.
        The root record is 0xFFFF when the table does not hold the root."""
        if self.codec.game_id == _lib.GAME_GRAPH:
            raise NoDescriptor("a stored table loads into a descriptor game only: the keys of a graph solve are "
                               "the host walk's numbering, which a table does not carry")
        self.n_positions, self.root_record = self.ctx.import_table(keys, records, self.root_key)
        return self.n_positions, self.root_record

    def load_statsdir(self, statsdir):
        """load() of every ``stats/<rank>/table.npz`` under `statsdir` (what ``-sd`` writes; a
        sharded solve's ranks each wrote their share).  The files must be of this solver's codec."""
        if self.codec.game_id == _lib.GAME_GRAPH:
            raise NoDescriptor("a stored table loads into a descriptor game only")
        from .persist import read_npz_tables
        keys, recs, meta = read_npz_tables(statsdir)
        mine = (self.codec.name, tuple(self.codec.params))
        if (meta.get("codec"), tuple(meta.get("params", ()))) != mine:
            raise ValueError("%s holds a table of codec %r with params %r; this solver's codec is %r with %r"
                             % (statsdir, meta.get("codec"), meta.get("params"), mine[0], mine[1]))
        return self.load(keys, recs)

    @property
    def value(self):
        return split_record(self.root_record)[0]

    @property
    def remoteness(self):
        return split_record(self.root_record)[1]

    def root_line(self):
        """The reference's root line (src/new_process.py:47-52)."""
        v, r = split_record(self.root_record)
        if v == DRAW:   # nobody can force an end: a move count has no meaning
            return to_str(v)
        return "%s in %d moves" % (to_str(v), r)

    def lookup(self, pos):
        rec = self.ctx.query([self.codec.key(pos)])[0]
        return split_record(rec)

    def table(self):
        """Sorted keys and u16 records of every solved position."""
        return self.ctx.export()

    def analysis(self):
        """Positions of the whole solve on this rank by value and remoteness: a (3, n_rem)
        uint64 array, rows WIN, LOSS, TIE (gamesmanmpi_amd/analysis.py).  The nodes of a graph
        solve with symmetry generators are orbit representatives, which the device counts
        once each: those (host-enumerated, small) graphs are weighted here by orbit size."""
        if self.codec.game_id == _lib.GAME_GRAPH and self.codec.gens:
            from . import analysis
            keys, recs = self.ctx.export()
            keep = recs != _lib.REC_DRAW   # DRAW has no row (draw_count)
            return analysis.from_records(recs[keep], [len(self.codec.members(k)) for k in keys[keep]])
        return self.ctx.histogram()

    def draw_count(self):
        """DRAW positions of the solve (0 unless it was loopy); orbit representatives are
        weighted by orbit size, as in analysis()."""
        if self.codec.game_id == _lib.GAME_GRAPH and self.codec.gens:
            keys, recs = self.ctx.export()
            return sum(len(self.codec.members(k)) for k in keys[recs == _lib.REC_DRAW])
        return self.ctx.draw_count()

    def verify(self, cap=64):
        """Check the solved table against the game rules on the device (gm_verify):
        (counts dict, up to `cap` offending keys)."""
        return self.ctx.verify(cap)

    def reach(self, positions=None, mover="all", other="all", max_plies=0, cap=0):
        """The positions reachable from `positions` (default: the root) when their mover follows
        policy `mover` and the opponent `other` ("all", "best", "first"), found on the device
        (gm_reach).  Returns the dict of gm_reach_out_t with "ply_counts" (positions first
        reached per ply), "share" (n over n_positions) and, with cap > 0, "positions": up to
        `cap` rows (position, value, remoteness, side bits), ascending by key.  The nodes of a
        graph solve with symmetry generators are orbit representatives: their counts are
        weighted by orbit size here, as find() weights them."""
        from . import reach as R
        starts = [self.codec.key(p) for p in ([self.root] if positions is None else positions)]
        pm, po = R.policy(mover), R.policy(other)
        weighted = self.codec.game_id == _lib.GAME_GRAPH and bool(self.codec.gens)
        want = max(int(cap), self.ctx.stats()["n_positions"]) if weighted else int(cap)
        out, pcs, keys, recs, sides = self.ctx.reach(starts, pm, po, max_plies, want)
        pcs = [int(x) for x in pcs]
        if weighted:
            w = {int(k): len(self.codec.members(int(k))) for k in keys}
            out["n"] = sum(w.values())
            out["n_mover"] = sum(w[int(k)] for k, s in zip(keys, sides) if s & 1)
            out["n_other"] = sum(w[int(k)] for k, s in zip(keys, sides) if s & 2)
            # a ply's pairs: what a search bounded at that ply adds to the one bounded a ply earlier
            seen, pcs = set(), []
            for d in range(out["plies"]):
                if d == 0:
                    pairs = {(int(k), 0) for k in starts if int(k) in w}
                else:
                    _, _, kd, _, sd = self.ctx.reach(starts, pm, po, d, want)
                    pairs = {(int(k), b) for k, s in zip(kd, sd) for b in (0, 1) if s >> b & 1}
                pcs.append(sum(w[k] for k, _ in pairs - seen))
                seen |= pairs
        out["ply_counts"] = pcs
        out["share"] = out["n"] / self.n_positions if self.n_positions else 0.0
        if cap:
            m = min(int(cap), len(recs))
            ks = [int(k) for k in keys[:m]] if self.ctx.words == 1 else [_lib.words_to_int(k) for k in keys[:m]]
            out["positions"] = [(self.codec.pos(k),) + split_record(r) + (int(s),)
                                for k, r, s in zip(ks, recs[:m], sides[:m])]
        return out

    def strategy(self, pos=None, side=None, first=False):
        """The weak solution inside the strong one: the positions that can occur from `pos`
        (default: the root) when one side plays perfectly -- every optimal move, or with
        first=True the one move the solver plays -- and the other side plays anything.  `side`
        is "mover" (the player to move at `pos`) or "other"; it defaults to the side that does
        not lose at `pos`: the mover for WIN / TIE / DRAW, the opponent for LOSS.  Returns
        reach()'s dict with "side" and "value" (of `pos`)."""
        pos = self.root if pos is None else pos
        value = self.lookup(pos)[0]
        if side is None:
            side = "other" if value == LOSS else "mover"
        if side not in ("mover", "other"):
            raise ValueError("side is 'mover' or 'other'")
        perfect = "first" if first else "best"
        out = self.reach([pos], mover=perfect if side == "mover" else "all",
                         other=perfect if side == "other" else "all")
        out["side"], out["value"] = side, value
        return out

    def moves(self, pos):
        """The moves at `pos` and what each is worth: rows (move, child position, value,
        remoteness) in the plugin's gen_moves order, and the row the solver would play (None at
        a primitive position)."""
        if self.module.primitive(pos) != UNDECIDED:
            return [], None
        labels = list(self.module.gen_moves(pos))
        if self.codec.game_id == _lib.GAME_GRAPH:
            # no device descriptor: the plugin's own moves, looked up by position
            kids = [self.codec.key(self.module.do_move(pos, m)) for m in labels]
            recs = self.ctx.query(kids)
            best = best_move(recs)[0]
        else:
            kids, recs, best = self.ctx.moves(self.codec.key(pos))
            if len(labels) != len(kids):   # a plugin that lists a move twice: number the children
                labels = list(range(len(kids)))
        rows = [(m, self.codec.pos(k)) + split_record(r) for m, k, r in zip(labels, kids, recs)]
        return rows, (rows[best] if best is not None else None)

    def annotate(self, positions):
        """moves() for many positions at once: a list with, per position, what moves(pos)
        returns, from one gm_moves call (Context.moves_batch).  A graph context is looked up by
        position, as moves() does -- its nodes are orbit representatives under symmetry
        generators, and its CSR lists each distinct child once where gen_moves may not -- with
        one batched query for all the children."""
        positions = list(positions)
        if self.codec.game_id == _lib.GAME_GRAPH:
            labels = [list(self.module.gen_moves(p)) if self.module.primitive(p) == UNDECIDED else None
                      for p in positions]
            kids = [[self.codec.key(self.module.do_move(p, m)) for m in ms] if ms is not None else []
                    for p, ms in zip(positions, labels)]
            flat = [k for ks in kids for k in ks]
            recs = self.ctx.query(flat) if flat else np.zeros(0, dtype=np.uint16)
            out, at = [], 0
            for ms, ks in zip(labels, kids):
                if ms is None:
                    out.append(([], None))
                    continue
                rs = recs[at:at + len(ks)]
                at += len(ks)
                best = best_move(rs)[0]
                rows = [(m, self.codec.pos(k)) + split_record(r) for m, k, r in zip(ms, ks, rs)]
                out.append((rows, rows[best] if best is not None else None))
            return out
        heads, ck, cr = self.ctx.moves_batch([self.codec.key(p) for p in positions])
        out = []
        for pos, h in zip(positions, heads):
            if self.module.primitive(pos) != UNDECIDED:
                out.append(([], None))
                continue
            if int(h["record"]) == _lib.REC_UNSOLVED:   # not in the table: gm_moves lists nothing, moves() expands
                out.append(self.moves(pos))
                continue
            first, count = int(h["first"]), int(h["count"])
            kids = ck[first:first + count]
            kids = [int(k) for k in kids] if self.ctx.words == 1 else [_lib.words_to_int(k) for k in kids]
            labels = list(self.module.gen_moves(pos))
            if len(labels) != len(kids):   # a plugin that lists a move twice: number the children
                labels = list(range(len(kids)))
            rows = [(m, self.codec.pos(k)) + split_record(r) for m, k, r in zip(labels, kids, cr[first:first + count])]
            out.append((rows, rows[int(h["best"])] if count else None))
        return out

    def find(self, spec_or_values, rem=None, cap=16, with_keys=False):
        """The positions with a given value and remoteness, selected on the device (gm_select).
        `spec_or_values` is a spec of gamesmanmpi_amd/find.py ("tie:9", "win,loss:2-5",
        "win:max") or an OR of _lib.SEL_* with `rem` None (any), one remoteness or (lo, hi).
        Returns (n, [(position, value, remoteness), ...]): n counts every match, the rows are
        up to `cap` of them ascending by key.  The nodes of a graph solve with symmetry
        generators are orbit representatives: they are expanded here with codec.members and
        every member counts, as in analysis()."""
        from . import find
        if isinstance(spec_or_values, (str, find.Spec)):
            spec = find.as_spec(spec_or_values)
            if spec.want_max:
                spec = find.resolve(spec, self.analysis())
        else:
            lo, hi = (0, find.ANY) if rem is None else (rem if isinstance(rem, (tuple, list)) else (rem, rem))
            spec = find.Spec(int(spec_or_values), int(lo), int(hi), False)
        if self.codec.game_id == _lib.GAME_GRAPH and self.codec.gens:
            n_rep = self.ctx.select(spec.values, spec.rem_lo, spec.rem_hi, 0)[0]
            _, keys, recs = self.ctx.select(spec.values, spec.rem_lo, spec.rem_hi, n_rep)
            n, rows, kept = 0, [], []
            for k, r in zip(keys, recs):
                members = self.codec.members(k)
                n += len(members)
                for p in members[:max(0, cap - len(rows))]:
                    rows.append((p,) + split_record(r))
                    kept.append(k)
        else:
            n, kept, recs = self.ctx.select(spec.values, spec.rem_lo, spec.rem_hi, cap)
            rows = [(self.codec.pos(k),) + split_record(r) for k, r in zip(kept, recs)]
        return (n, rows, kept) if with_keys else (n, rows)

    def line(self, pos=None, max_plies=0x4000):
        """The principal variation from `pos` (default the root): rows (move, position, value,
        remoteness), the first with move None, each next one the row moves() marks as the
        solver's choice, the last a primitive position.  From a DRAW position of a loopy solve
        nobody ends the game: the line stops on the first position it repeats, or after
        `max_plies` moves."""
        pos = self.root if pos is None else pos
        rows, seen, move = [], set(), None
        while True:
            v, r = self.lookup(pos)
            rows.append((move, pos, v, r))
            if self.module.primitive(pos) != UNDECIDED or len(rows) > max_plies:
                break
            if v == DRAW:
                k = self.codec.key(pos)
                if k in seen:
                    break
                seen.add(k)
            _, best = self.moves(pos)
            if best is None:
                break
            move, pos = best[0], best[1]
        return rows

    def close(self):
        self.ctx.close()


def dump_table(path, keys, records, meta=None):
    """Write a solved table as ``.npz`` (sorted u64 keys, u16 records)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, keys=keys, records=records, meta=str(meta or {}))
