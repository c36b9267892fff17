"""The planned end of phase 1 without a GPU (wfmash_amd/csrc/wfa_plan.h through wfmh_test_planned_meet): a job whose score is known ends its
first loop at a state fixed by that score, and phase 2 from there must find what the reference finds from its own trigger.

Against the oracle, for every child of the roots of tests/tile_path_cases.py's family, of the selections the GPU test runs and of the pairs
that meet inside a long gap (tests/planned_meet_cases.py), taken as oracle.align_comp's inputs:
  * the planned state lies on the alternating track: sr = sf - last_fwd, last_fwd in {0, 1};
  * sf + sr <= score_forward + score_reverse of pyoracle.find_breakpoint on that child -- no test before the planned state can be the one that
    takes the breakpoint (a hit needs the sum of the two rows' scores to reach the breakpoint's);
  * the walk of phase 2 from there stays within one round: find_breakpoint_rounds with a cut after every test counts the tests the reference
    makes from ITS trigger (pyoracle.meet_point), and every state between the two is one test more or one fewer.
The cases kept are those for which the oracle's own walk fits a round (all of them do; the filter is asserted to drop nothing).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import planned_meet_cases as PM
import tile_path_cases as TC
from oracle import pyoracle as O

SUB_NONE = 1 << 29
INT_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def _lib():
    from wfmash_amd import capi
    lib = capi.load()
    assert "wfmh_test_planned_meet" in capi.HOST_EXPORTS
    lib.wfmh_test_planned_meet.restype = C.c_int
    lib.wfmh_test_planned_meet.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    return lib


def _ask(rows):
    """rows of (score_rem, cb, ce, second, sub, fits, tile_it, grown, packed, s_keep, T) at the default penalties -> rows of the hook's 8 results"""
    a = np.array([list(O.DEFAULT_PEN) + list(r) for r in rows], dtype=np.int64)
    assert a.shape[1] == 16
    out = np.zeros((len(rows), 8), dtype=np.int64)
    assert _lib().wfmh_test_planned_meet(a.ctypes.data, len(rows), out.ctypes.data) == 0
    return out


@functools.lru_cache(maxsize=None)
def _jobs():
    """every bialign job below the roots of the three sets, once"""
    roots = [(c.p, c.t) for c in TC.select(100)][::6] + list(PM.select(100)) + list(PM.select(32)) + list(PM.gap_pairs())
    seen, out = set(), []
    for p, t in roots:
        for j in PM.descendants(p, t):
            key = (j.p, j.t, j.cb, j.ce)
            if key not in seen:
                seen.add(key)
                out.append(j)
    return out


def test_the_sets_reach_gap_components_and_both_children():
    jobs = _jobs()
    assert len(jobs) >= 100
    kinds = {(j.cb != 0, j.ce != 0, j.second) for j in jobs}
    # a first child that ends in the gap its parent's breakpoint cut, a second child that begins in it, and jobs that inherited a gap component
    # at the far end (the child of a child)
    assert (False, True, 0) in kinds and (True, False, 1) in kinds, kinds
    assert (False, True, 1) in kinds or (True, False, 0) in kinds, kinds
    assert {PM.gopen(j.ce) for j in jobs if not j.second} >= {0, 8, 24}, "cuts in M, in a one-piece gap and in a two-piece gap"


def test_planned_state_against_the_oracle():
    jobs = _jobs()
    got = _ask([(j.score, j.cb, j.ce, j.second, j.score + 56, 1, 1, 0, 1, 0, 100) for j in jobs])
    kept = 0
    for j, g in zip(jobs, got):
        total, sf, sr, lf = (int(x) for x in g[:4])
        assert (sf, sr, lf) == PM.planned(j), (j.score, j.cb, j.ce, j.second, g)
        assert total == sf + sr and lf in (0, 1) and sr == sf - lf and sf >= 1, g               # on the alternating track
        rc, bp, _ = O.find_breakpoint(j.p, j.t, j.cb, j.ce)
        assert rc == 0
        assert sf + sr <= bp.score_forward + bp.score_reverse, (sf, sr, bp.score_forward, bp.score_reverse, j.cb, j.ce, j.second)
        # the child's own optimum is exactly what the plan subtracts from: the sum is the first at which a test CAN hit
        assert sf + sr == bp.score, (sf, sr, bp.score, j.cb, j.ce, j.second)
        # the oracle's own walk: tests from its trigger; from the planned state one more (fewer) per state the plan lies before (behind) it
        rc1, bp1, rounds1 = O.find_breakpoint_rounds(j.p, j.t, PM.P2TESTS, -1, j.cb, j.ce)
        assert rc1 == 0
        if rounds1 != 1:
            continue
        kept += 1
        rc2, _, tests = O.find_breakpoint_rounds(j.p, j.t, 1, -1, j.cb, j.ce)  # a cut before every test but the first: rounds = tests
        msf, msr, _ = O.meet_point(j.p, j.t, None, j.cb, j.ce)
        assert rc2 == 0 and msf + msr > 0
        from_plan = tests + (msf + msr) - (sf + sr)
        assert 0 < from_plan <= PM.P2TESTS, (tests, msf + msr, sf + sr, j.cb, j.ce, j.second)
    assert kept == len(jobs), (kept, len(jobs))


def test_block_of_the_planned_end():
    rows, want = [], []
    for T in (100, 32, 128):
        for s in list(range(251, 700, 7)) + [2 * T * q + d for q in (2, 3) for d in (-1, 0, 1, 2, 3)]:
            rows.append((s, 0, 0, 0, s + 56, 1, 1, 0, 1, 0, T))
            sf, sr = (s + 1) // 2, s // 2
            b = (sf - 1) // T
            want.append((b * T, sf - b * T, sr - b * T))
    got = _ask(rows)
    for r, g, w in zip(rows, got, want):
        assert tuple(int(x) for x in g[4:7]) == w, (r, g, w)
        assert 1 <= g[5] <= r[-1] and 0 <= g[6] <= r[-1] and g[5] - g[6] == g[3]


def test_eligibility():
    S, T = 1000, 100  # planned end at (500, 500): block 400, tf = 100

    def one(**kw):
        d = dict(score=S, cb=0, ce=0, second=0, sub=S + 56, fits=1, tile_it=1, grown=0, packed=1, s_keep=0, T=T)
        d.update(kw)
        return int(_ask([(d["score"], d["cb"], d["ce"], d["second"], d["sub"], d["fits"], d["tile_it"], d["grown"], d["packed"], d["s_keep"], d["T"])])[0][7])
    assert one() == 1
    assert one(sub=SUB_NONE) == 0          # a child without the bound its parent's score gives (the unbounded configuration)
    assert one(score=INT_MAX, sub=5000) == 0  # a root, even a bounded one: its score is a guess
    assert one(packed=0) == 0              # the byte kernel's
    assert one(grown=1) == 0 and one(tile_it=0) == 0 and one(fits=0) == 0
    # the block of the planned end is not the first one after a restore
    assert one(s_keep=300) == 1 and one(s_keep=200) == 1 and one(s_keep=400) == 0
    assert one(score=1002, s_keep=400) == 1  # (501, 501): block 500


def test_gpu_selections_hold_their_classes():
    """what tests/test_planned_meet_gpu.py runs: every (block, tf) asked for is the planned end of some job below the selection's roots"""
    for T in (100, 32):
        roots = PM.select(T)
        assert 0 < len(roots) <= 40, len(roots)
        assert all(2000 <= len(p) <= 4000 and 2000 <= len(t) <= 4000 for p, t in roots)
        missing = set(PM.wanted(T)) - PM.covered(roots, T)
        assert not missing, (T, sorted(missing))
