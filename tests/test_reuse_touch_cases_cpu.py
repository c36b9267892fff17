"""The family of tests/reuse_touch_cases.py without a GPU: what it covers, and the theorem parent reuse rests on (DESIGN.md section 5,
"When a kept row is the child's row"), from the oracle alone.

Coverage: per block length, children whose every possible keep touches their box (in both directions, with a breakpoint in a gap
component, with the side of the box touched and not its corner), children no keep of which touches (down to the nearest misses), few
in between.  The theorem: where no kept cell touches, the child's own rows hold the parent's cells; where one touches they do not --
so a touch the kernel missed would change the rows a child goes on from, and tests/test_reuse_touch_gpu.py can fail.
"""
import pytest

import reuse_touch_cases as R
from oracle import pyoracle as O


def _of(T, name, di):
    return [(ri, c) for ri, d, c in R.table(T) if d == di and c.name == name]


def test_the_children_split_the_roots_scores():
    for r in R.roots():
        bp = r.bp
        assert bp.score_forward + bp.score_reverse - R.gap_open(bp.component) == bp.score == r.score, r.spec
        a, b = r.children
        assert len(a.p) + len(b.p) == len(r.p) and len(a.t) + len(b.t) == len(r.t)
        assert (a.score, b.score) == (bp.score_forward, bp.score_reverse)
        assert 1200 <= max(len(r.p), len(r.t)) <= 8000 and r.score <= 7000, (r.spec, len(r.p), len(r.t), r.score)
    rc, _, score, _ = O.align_biwfa(R.roots()[0].p, R.roots()[0].t)   # (the bounded search's score is the alignment's)
    assert rc == 0 and score == R.roots()[0].score


@pytest.mark.parametrize("T", R.TS)
def test_coverage(T):
    tb = R.table(T)
    print("T", T, {(n, d): len(_of(T, n, d)) for n in ("touch", "clear", "depends") for d in (0, 1)})
    for di in (0, 1):
        touch, clear = _of(T, "touch", di), _of(T, "clear", di)
        assert len(touch) >= 8, (T, di, len(touch))
        assert any(R.roots()[ri].bp.component != O.COMP["M"] for ri, _ in touch), (T, di)
        assert any(R.side_only(ri, di, T) for ri, _ in touch), (T, di)
        assert len(clear) >= 8, (T, di, len(clear))
        near = [(ri, c.margin_hi, c.least) for ri, c in clear if 1 <= c.margin_hi <= 4]
        print("T", T, "direction", di, "nearest misses (root, margin at s_hi, least margin):", near)
        assert near, (T, di)
        # to the base: a child every keep of which touches with its furthest cell ON the wall (v == hmax_c: `>` for `>=` would resume it), and one
        # every keep of which stops one base short (a wall one too low would give it up)
        assert any(c.most == 0 and c.least == 0 for _, c in touch), (T, di)
        assert any(c.most == 1 and c.least == 1 for _, c in clear), (T, di)
    assert 4 * sum(c.name == "depends" for _, _, c in tb) <= len(tb)
    # every root hands both children a keep's worth of score under either block length, and some carry an N
    assert len(tb) == 2 * len(R.roots())
    assert sum(b"N" in r.p for r in R.roots()) >= 4
    least = min(c.least for _, _, c in tb if c.name == "clear")
    print("T", T, "smallest positive margin:", least)
    assert least >= 1


def _differing(child, s, sub_child, sub_parent, sub_range):
    """cells of the rows a keep at s holds, over the child's range under the bound sub_range, where the child's own run (under sub_child; < 0:
    none) and its parent's (under sub_parent) differ -> (cells compared, cells that differ)"""
    pl, tl = len(child.p), len(child.t)
    pk, poff, _ = O.forward_rows(child.par_p, child.par_t, s, sub=sub_parent)
    ck, coff, _ = O.forward_rows(child.p, child.t, s, sub=sub_child)
    n = bad = 0
    for comp, back in R.KEEP:
        lo, hi = R.rng(pl, tl, sub_range, s - back)
        if s - back < 0 or hi < lo:
            continue
        a, b = poff[comp, back, lo - pk:hi + 1 - pk], coff[comp, back, lo - ck:hi + 1 - ck]
        assert len(a) == len(b) == hi - lo + 1
        n += hi - lo + 1
        bad += int((a != b).sum())
    return n, bad


@pytest.mark.parametrize("T", R.TS)
def test_a_keep_that_does_not_touch_is_the_childs_own_rows(T):
    cells = 0
    for ri, di, c in R.table(T):
        if c.name != "clear":
            continue
        root, child = R.roots()[ri], R.roots()[ri].children[di]
        # the child without a bound against the parent without one, over the range the product gives the child (its score and the slack) ...
        n, bad = _differing(child, c.s_hi, -1, -1, child.score + R.SUB_SLACK)
        assert n > 0 and bad == 0, (T, ri, di, n, bad)
        # ... and the child cut at its own score against the parent cut at its own, over the range that leaves
        n2, bad = _differing(child, c.s_hi, child.score, root.score, child.score)
        assert bad == 0, (T, ri, di, n2, bad)
        cells += n + n2
    print("T", T, "cells compared:", cells)


@pytest.mark.parametrize("T", R.TS)
def test_a_keep_that_touches_is_not(T):
    for di in (0, 1):
        found = []
        for ri, c in _of(T, "touch", di)[:4]:
            child = R.roots()[ri].children[di]
            n, bad = _differing(child, c.s_hi, -1, -1, child.score + R.SUB_SLACK)
            if bad:
                found.append((ri, n, bad))
        print("T", T, "direction", di, "must-touch children whose own rows differ from the keep (root, cells, differing):", found)
        assert found, (T, di)
