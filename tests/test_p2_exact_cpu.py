"""The exact walk of phase 2 without a GPU: the rule wfa_p2_exact_kernel implements ("the exact walk"), as a model in
Python over the oracle's own rows, against the oracle's breakpoint.

A job below the roots enters phase 2 at its planned end X (tests/planned_meet_cases.py, planned): sf + sr = S_own, its optimal score.  The
reference takes a hit only when it is strictly cheaper than the best in hand and nothing is cheaper than S_own, so its final breakpoint is the
first hit of score exactly S_own in its walk order.  At the test u states behind X a pair (row s1 - i of the other direction, component c) has
that score iff i = u - gopen(c): one row per component.  The model walks the track from X, looks at those pairs alone, takes the smallest
diagonal of the tested row on which the offsets meet, and stops at the first test with a hit; among a test's hits it takes the reference's
order, i ascending, then D2, I2, D1, I1, M.

Rows: pyoracle.forward_rows, the reverse direction's from the reversed sequences; two windows a direction cover the scores sd - 25 .. sd + 26.
For every job below the roots of the sets the GPU test runs (planned_meet_cases.select(100), select(32), gap_pairs(), and the short gaps of
tests/p2_exact_cases.py, without which no breakpoint below a root falls into I1 or D1) and of the roots of tests/reuse_touch_cases.py the model must give pyoracle.find_breakpoint's score, score_forward, score_reverse, component and diagonal, within
scope - 1 + max(o1, o2) + 1 = 50 tests.
"""
import collections
import functools

import numpy as np

import p2_exact_cases as XC
import planned_meet_cases as PM
import reuse_touch_cases as RT
from oracle import pyoracle as O

SCOPE = 26                 # rows of the other direction a test looks back over at the default penalties
REACH = SCOPE - 1 + max(O.DEFAULT_PEN[1], O.DEFAULT_PEN[3])   # the last test u at which a pair of score S_own has 0 <= i < scope
ORDER = (O.COMP["D2"], O.COMP["I2"], O.COMP["D1"], O.COMP["I1"], O.COMP["M"])   # the reference's order among the components of one row

Hit = collections.namedtuple("Hit", "u score score_forward score_reverse component k_forward offset_forward")


class Rows:
    """one direction's rows sd - 25 .. sd + 26, addressable by score and diagonal"""

    def __init__(self, p, t, sd, comp_begin):
        self.sd = sd
        self.kmin, self.off, self.rng = O.forward_rows(p, t, [sd, sd + O.ROWS], comp_begin)

    def row(self, comp, s):
        """-> (lo, hi, offsets over lo .. hi); lo > hi: no row"""
        w, back = (0, self.sd - s) if s <= self.sd else (1, self.sd + O.ROWS - s)
        assert 0 <= back < O.ROWS
        lo, hi = (int(x) for x in self.rng[w, comp, back])
        if lo > hi:
            return lo, hi, None
        return lo, hi, self.off[w, comp, back, lo - self.kmin:hi + 1 - self.kmin].astype(np.int64)


def track_test(sf, sr, last_fwd, u):
    """test u of the track behind (sf, sr): the direction that stepped last is tested first, then the two alternate -> (d0, s0, s1)"""
    first = 0 if last_fwd else 1
    a, b = (sf, sr) if first == 0 else (sr, sf)
    if u % 2 == 0:
        return first, a + u // 2, b + u // 2
    return first ^ 1, b + (u + 1) // 2, a + (u - 1) // 2


def exact_walk(job):
    """-> Hit of the model, None: no pair of score S_own met within the reach"""
    sf, sr, lf = PM.planned(job)
    exact = sf + sr
    pl, tl = len(job.p), len(job.t)
    kinv = tl - pl
    rows = (Rows(job.p, job.t, sf, job.cb), Rows(job.p[::-1], job.t[::-1], sr, job.ce))
    for u in range(REACH + 1):
        d0, s0, s1 = track_test(sf, sr, lf, u)
        found = []
        for oi, cc in enumerate(ORDER):
            i = s0 + s1 - PM.gopen(cc) - exact
            if not (0 <= i < SCOPE and s1 - i >= 0):
                continue
            si = s1 - i
            lo0, hi0, r0 = rows[d0].row(cc, s0)
            lo1, hi1, r1 = rows[d0 ^ 1].row(cc, si)
            if r0 is None or r1 is None:
                continue
            ka, kb = max(lo0, kinv - hi1), min(hi0, kinv - lo1)
            if ka > kb:
                continue
            a = r0[ka - lo0:kb + 1 - lo0]
            b = r1[kinv - kb - lo1:kinv - ka + 1 - lo1][::-1]   # the mirrored diagonals, in the tested row's order
            meet = np.nonzero(a + b >= tl)[0]
            if len(meet):
                found.append((i, oi, cc, si, ka + int(meet[0])))
        if found:
            i, _, cc, si, k0 = min(found)
            if d0 == 0:
                s_f, s_r, kf = s0, si, k0
            else:
                s_f, s_r, kf = si, s0, kinv - k0
            lo, _, r = rows[0].row(cc, s_f)
            return Hit(u, exact, s_f, s_r, cc, kf, int(r[kf - lo]))
    return None


def _below(p, t, bp=None):
    """PM.descendants with every job's own breakpoint (one search of the oracle per job) -> [(Job, Breakpoint)]; bp: the root's, if known"""
    out = []
    if bp is None:
        rc, bp, _ = O.find_breakpoint(p, t)
        assert rc == 0
    todo = [(PM.Job(p, t, PM.C_M, PM.C_M, None, 0, 0), bp)]
    while todo:
        j, b = todo.pop()
        for c in PM.children(j.p, j.t, j.cb, j.ce, b, j.depth):
            if len(c.p) and len(c.t) and c.score > PM.MIN_SCORE:
                rc, cb, _ = O.find_breakpoint(c.p, c.t, c.cb, c.ce)
                assert rc == 0
                out.append((c, cb))
                todo.append((c, cb))
    return out


@functools.lru_cache(maxsize=None)
def _jobs():
    """every bialign job below the roots of the sets, once, with pyoracle.find_breakpoint's answer (the roots of tests/reuse_touch_cases.py come
    with their breakpoint)"""
    roots = [(p, t, None) for p, t in list(PM.select(100)) + list(PM.select(32)) + list(PM.gap_pairs()) + XC.short_gap_pairs()]
    roots += [(r.p, r.t, r.bp) for r in RT.roots()]
    seen, out = set(), []
    for p, t, bp in roots:
        for j, b in _below(p, t, bp):
            key = (j.p, j.t, j.cb, j.ce)
            if key not in seen:
                seen.add(key)
                out.append((j, b))
    return out


@functools.lru_cache(maxsize=None)
def _walks():
    return [exact_walk(j) for j, _ in _jobs()]


def test_the_model_finds_the_oracles_breakpoint():
    jobs, walks = _jobs(), _walks()
    assert len(jobs) >= 200
    for (j, bp), w in zip(jobs, walks):
        assert w is not None, (len(j.p), len(j.t), j.cb, j.ce, j.score, bp.score)
        assert w.u <= REACH and w.u < 50
        got = (w.score, w.score_forward, w.score_reverse, w.component, w.k_forward, w.offset_forward)
        want = (bp.score, bp.score_forward, bp.score_reverse, bp.component, bp.k_forward, bp.offset_forward)
        assert got == want, (got, want, w.u, len(j.p), len(j.t), j.cb, j.ce, j.score)


def test_the_family_covers_components_and_depths():
    walks = [w for w in _walks() if w is not None]
    comps = collections.Counter(w.component for w in walks)
    assert all(comps[c] > 0 for c in range(5)), comps           # a breakpoint in each of M, I1, I2, D1, D2
    us = collections.Counter(w.u for w in walks)
    assert us[0] > 0, us                                          # the pair at X itself (M, i = 0)
    assert sum(n for u, n in us.items() if 1 <= u <= 10) > 0, us  # a few states behind it
    assert sum(n for u, n in us.items() if u >= 24) > 0, us       # a two-piece gap: i = u - o2
    # a hit in a gap component lies o1 / o2 tests behind X at the least
    for w in walks:
        assert w.u >= PM.gopen(w.component), w
