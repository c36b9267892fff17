"""The wave-uniform interior test of the packed tile kernel without a GPU (wfmash_amd/csrc/wfa_rows.h, rng_interior, through
wfmh_test_tile_interior): "every diagonal of a span lies inside its row at every score of an interval", decided from the two end rows,
against brute force over every score and every diagonal with rng_lo / rng_hi (the same hook returns them for one score at a time).

A wave that passes the test loads and stores its snapshot rows without a range test per row, so a false positive is a wrong result; a
false negative only costs speed.  The argument in wfa_rows.h says the test is exact, and that is what is asserted: the predicate equals
the brute force on every geometry, so the share of false negatives is 0 everywhere, not only on spans strictly inside."""
import ctypes as C
import random

import numpy as np
import pytest

from wfmash_amd import capi

SUB_NONE = 1 << 29


@pytest.fixture(scope="module")
def L():
    lib = capi.load()
    assert "wfmh_test_tile_interior" in capi.HOST_EXPORTS
    lib.wfmh_test_tile_interior.restype = C.c_int
    lib.wfmh_test_tile_interior.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    return lib


def ask(L, rows):
    q = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 7)
    out = np.zeros((len(q), 3), dtype=np.int32)
    assert L.wfmh_test_tile_interior(q.ctypes.data, len(q), out.ctypes.data) == 0
    return out


def brute(L, geoms):
    """per geometry: is every diagonal of [ka, kb] inside [rng_lo(s), rng_hi(s)] at every s of [sa, sb] -- one hook row per score"""
    rows, owner = [], []
    for i, (pl, tl, sub, ka, kb, sa, sb) in enumerate(geoms):
        for s in range(sa, sb + 1):
            rows.append((pl, tl, sub, ka, kb, s, s))
            owner.append(i)
    out = ask(L, rows)
    ok = np.ones(len(geoms), dtype=bool)
    q = np.array(rows, dtype=np.int64)
    inside = (q[:, 3] >= out[:, 1]) & (q[:, 4] <= out[:, 2])
    np.logical_and.at(ok, np.array(owner), inside)
    return ok


def py_lo(pl, tl, sub, s):
    return max(-pl, -s, (tl - pl) - sub + s)


def py_hi(pl, tl, sub, s):
    return min(tl, s, (tl - pl) + sub - s)


def geometries(seed, n):
    """(pl, tl, sub, ka, kb, sa, sb), ka <= kb and sa <= sb: small problems, so that the brute force stays cheap, drawn around every edge
    a row's range has -- the triangle, the box [-pl, tl], the two sides of a score bound's cone -- and around score 25"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        kind = rng.randrange(8)
        pl, tl = rng.randrange(1, 900), rng.randrange(1, 900)
        if kind in (1, 5):  # the end diagonal tl - pl far from 0
            pl, tl = (rng.randrange(20, 120), rng.randrange(600, 1500)) if rng.random() < 0.5 else (rng.randrange(600, 1500), rng.randrange(20, 120))
        kinv = tl - pl
        sub = SUB_NONE if kind in (0, 2, 3) else abs(kinv) + rng.randrange(0, 400)  # a bound below |kinv| admits no alignment; at it, it binds hardest
        span = rng.choice([1, 2, 64, 127, 128, 128, 128, 200])
        nsc = rng.choice([1, 2, 26, 26, 26, 40])
        smax = min(sub, pl + tl + 60) if sub != SUB_NONE else pl + tl + 60
        sb = rng.randrange(0, smax + 30)
        if kind == 3:
            sb = rng.randrange(0, 60)  # scores below 25: the first rows of the interval do not exist
        if kind in (5, 6):
            sb = max(0, sub - rng.randrange(0, 200))  # the cone's shrinking side
        sa = sb - nsc + 1
        lo_a, hi_a, lo_b, hi_b = py_lo(pl, tl, sub, max(sa, 0)), py_hi(pl, tl, sub, max(sa, 0)), py_lo(pl, tl, sub, sb), py_hi(pl, tl, sub, sb)
        anchor = rng.choice([-pl, tl, lo_a, hi_a, lo_b, hi_b, kinv, (max(lo_a, lo_b) + min(hi_a, hi_b)) // 2, rng.randrange(-pl - 50, tl + 50)])
        ka = anchor + rng.choice([0, 0, 1, -1, -span + 1, -span, -span + 2, -span // 2, 3, -3])  # at, across and beside the edge
        out.append((pl, tl, sub, ka, ka + span - 1, sa, sb))
    return out


def test_hook_returns_the_rows_ranges(L):
    geoms = geometries(11, 400)
    out = ask(L, geoms)
    for (pl, tl, sub, ka, kb, sa, sb), o in zip(geoms, out):
        assert (int(o[1]), int(o[2])) == (py_lo(pl, tl, sub, sa), py_hi(pl, tl, sub, sa))


def test_interior_predicate_is_the_brute_force(L):
    geoms = geometries(12, 6000)
    pred = ask(L, geoms)[:, 0].astype(bool)
    ref = brute(L, geoms)
    fp = [g for g, p, r in zip(geoms, pred, ref) if p and not r]
    fn = [g for g, p, r in zip(geoms, pred, ref) if r and not p]
    assert not fp, ("false positive", fp[:5], len(fp))
    assert not fn, ("false negative", fn[:5], len(fn))
    # every kind of answer is in the sample, with and without a bound, below score 25 and beyond it
    g = np.array(geoms, dtype=np.int64)
    for name, sel in (("no bound", g[:, 2] == SUB_NONE), ("bound", g[:, 2] != SUB_NONE), ("first score below 0", g[:, 5] < 0), ("first score >= 0", g[:, 5] >= 0),
                      ("far end diagonal", np.abs(g[:, 1] - g[:, 0]) > 400), ("shrinking side", (g[:, 2] != SUB_NONE) & (g[:, 6] > g[:, 2] - 200))):
        assert sel.sum() > 50, name
        assert (~ref[sel]).sum() > 5, name
        if name != "first score below 0":
            assert ref[sel].sum() > 5, name
    assert not ref[g[:, 5] < 0].any()  # a row of a negative score holds no cell


def test_spans_strictly_inside_pass(L):
    """spans with a diagonal to spare on either side at both end rows: all pass (no false negative), and moving such a span across either end
    of the narrower end row makes it fail"""
    rng = random.Random(13)
    inside, across = [], []
    while len(inside) < 1500:
        pl, tl = rng.randrange(200, 2500), rng.randrange(200, 2500)
        sub = SUB_NONE if rng.random() < 0.5 else abs(tl - pl) + rng.randrange(300, 900)
        sb = rng.randrange(140, min(sub, pl + tl))
        sa = sb - 25
        lo, hi = max(py_lo(pl, tl, sub, sa), py_lo(pl, tl, sub, sb)), min(py_hi(pl, tl, sub, sa), py_hi(pl, tl, sub, sb))
        if hi - lo < 131:
            continue
        ka = rng.randrange(lo + 1, hi - 128 + 1)
        inside.append((pl, tl, sub, ka, ka + 127, sa, sb))
        across.append((pl, tl, sub, lo - 1, lo + 126, sa, sb))
        across.append((pl, tl, sub, hi - 126, hi + 1, sa, sb))
    assert ask(L, inside)[:, 0].all() and brute(L, inside[:300]).all()
    assert not ask(L, across)[:, 0].any() and not brute(L, across[:300]).any()
