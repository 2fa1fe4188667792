"""The four engines that hold the subtraction game as 1-byte codes read their tables through
one host side (csrc/byte_tables.hpp).  One small 8-heap solve on each of them -- the box
engine, its split over 2 and 4 virtual ranks, the block engine and its partition over 4
virtual ranks -- compared against the oracle and against each other: query, digest, poke, and
the one place where the block engine differs on purpose (code 0 is a position not held).

Root 0x11132345: 11,520 positions in 8 boxes, more than one box along two A heaps and one B
heap, so a box index is not the key and the owner maps of the split engines are not trivial.
"""
import numpy as np
import pytest

from conftest import digest as table_digest

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, GMError, _lib  # noqa: E402

SUB = 5
ROOT = 0x11132345
REGION = 11520
LOSS_IN_0 = 1 << 14
TIE_IN_1 = (2 << 14) | 1
GM_E_ARG, GM_E_KEY = -1, -10
KEY = 0x01121212          # an interior position of the region
OUTSIDE = (ROOT + 1, 1 << 32, 2 ** 64 - 1)   # heap 0 above the root's; no 8-heap key; no key at all
ENGINES = {
    "dense_box": {},
    "dist_box2": {"virtual_ranks": 2},
    "dist_box4": {"virtual_ranks": 4},
    "dense_sub": {"sub_interleave": 10},
    "dist_sub4": {"sub_interleave": 10, "virtual_ranks": 4},
}


@pytest.fixture(scope="module")
def ref(oracle):
    keys, recs = oracle.solve(SUB, (8,), ROOT)
    assert len(keys) == REGION
    return keys, recs


@pytest.fixture(scope="module")
def solved():
    """Every engine's context, solved from ROOT.  A test that pokes puts the record back."""
    ctxs = {}
    for name, opts in ENGINES.items():
        ctx = Context(SUB, (8,), device=0)
        for k, v in opts.items():
            ctx.set_option(getattr(_lib, "OPT_" + k.upper()), v)
        n, _ = ctx.solve(ROOT)
        assert n == REGION
        assert ctx.stats()["engine"] == (_lib.ENGINE_DIST_DENSE if "virtual_ranks" in opts else _lib.ENGINE_DENSE)
        ctxs[name] = ctx
    yield ctxs
    for ctx in ctxs.values():
        ctx.close()


def test_query_region_and_outside(solved, ref):
    keys, recs = ref
    ask = np.concatenate([keys, np.array(OUTSIDE, dtype=np.uint64)])
    want = np.concatenate([recs, np.full(len(OUTSIDE), _lib.REC_UNSOLVED, dtype=np.uint16)])
    for name, ctx in solved.items():
        assert np.array_equal(ctx.query(ask), want), name


def test_digest_is_the_oracle_tables(solved, ref):
    want = (table_digest(*ref), REGION)
    for name, ctx in solved.items():
        assert ctx.digest() == want, name


def test_poke_checks_the_key_then_the_record(solved, ref):
    keys, recs = ref
    own = int(recs[np.searchsorted(keys, KEY)])
    assert own != LOSS_IN_0
    for name, ctx in solved.items():
        for key in OUTSIDE:
            with pytest.raises(GMError) as e:
                ctx.poke(key, TIE_IN_1)      # not a stored position: the key is refused before the record
            assert e.value.code == GM_E_KEY, name
        with pytest.raises(GMError) as e:
            ctx.poke(KEY, TIE_IN_1)          # the 1-byte codes hold no TIE
        assert e.value.code == GM_E_ARG, name
        assert ctx.query([KEY])[0] == own, name
        ctx.poke(KEY, LOSS_IN_0)
        assert ctx.query([KEY])[0] == LOSS_IN_0, name
        ctx.poke(KEY, own)
        assert ctx.query([KEY])[0] == own, name


def test_code_0_is_a_hole_on_the_block_engine_only(solved, ref):
    """gm_import leaves code 0 where a table has no position, and only the block engine imports:
    its digest skips code 0, the box engine's counts every position of the region."""
    keys, recs = ref
    own = int(recs[np.searchsorted(keys, KEY)])
    whole = table_digest(*ref)
    for name, count in (("dense_sub", REGION - 1), ("dense_box", REGION)):
        ctx = solved[name]
        ctx.poke(KEY, _lib.REC_UNSOLVED)
        d, n = ctx.digest()
        assert n == count and d != whole, name
        assert ctx.query([KEY])[0] == _lib.REC_UNSOLVED, name
        ctx.poke(KEY, own)
        assert ctx.digest() == (whole, REGION), name
