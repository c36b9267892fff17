"""Jobs of the BiWFA recursion whose score is known, and where their planned end of phase 1 falls in a tile block (shared by
tests/test_planned_meet_cpu.py and tests/test_planned_meet_gpu.py).

A child of the recursion comes with the score its parent's search credited it with (Node::score_rem), and wfa_plan.h's planned_meet says
at which state (sf, sr) of the reference's alternating track its phase 1 may end without a search.  Everything here is the oracle's: the
recursion is wavefront_bialign's (oracle/wfa2p.c, bialign_rec) walked with pyoracle.find_breakpoint, a job's children are the inputs of
oracle.align_comp, and which pairs go into a selection is decided by the oracle's breakpoints alone.

Only jobs with a score above 250 stay bialign jobs (BIALIGN_FALLBACK_MIN_SCORE), so a planned end lies at sf >= 126: at T = 100 in block 1
from tf = 26 on and in every later block, at T = 32 from block 3 on -- blocks 0 to 2 hold no planned end there, the selection takes 3 to 5.
"""
import collections
import functools

import tile_path_cases as TC
from oracle import pyoracle as O
from wfmash_amd import synth

MIN_SCORE = 250          # BIALIGN_FALLBACK_MIN_SCORE: a child at or below it is a base job
P2TESTS = 64             # 2 * P2K (wfa_device.h): the tests of one round of phase 2
C_M = 0

Job = collections.namedtuple("Job", "p t cb ce score second depth")  # a bialign job below a root: align_comp's inputs, Node::score_rem, which child it is


def gopen(comp, pen=None):
    pn = tuple(pen or O.DEFAULT_PEN)
    return 0 if comp == C_M else (pn[1] if comp in (1, 3) else pn[3])


def children(p, t, cb, ce, bp, depth):
    v, h = bp.offset_forward - bp.k_forward, bp.offset_forward
    return [Job(p[:v], t[:h], cb, bp.component, bp.score_forward, 0, depth + 1),
            Job(p[v:], t[h:], bp.component, ce, bp.score_reverse, 1, depth + 1)]


def descendants(p, t, pen=None):
    """-> [Job]: every job below the root (p, t) that the recursion hands to the breakpoint search again: both sequences non-empty, score > 250"""
    out, todo = [], [Job(p, t, C_M, C_M, None, 0, 0)]
    while todo:
        j = todo.pop()
        rc, bp, _ = O.find_breakpoint(j.p, j.t, j.cb, j.ce, pen)
        if rc != 0:
            continue  # (the directions' end reached at once: a base job)
        for c in children(j.p, j.t, j.cb, j.ce, bp, j.depth):
            if len(c.p) and len(c.t) and c.score > MIN_SCORE:
                out.append(c)
                todo.append(c)
    return out


def planned(job, pen=None):
    """the planned end as the test derives it (not the code under test): sf + sr = score - the opening of the gap the parent's breakpoint cut"""
    s = job.score - gopen(job.cb if job.second else job.ce, pen)
    return (s + 1) // 2, s // 2, s & 1


def block_class(sf, sr, T):
    b = (sf - 1) // T
    return b, sf - b * T, sr - b * T


def wanted(T):
    """(block, tf) a selection has to hold: tf in {1, 25, 26, 27, T - 1, T} of three consecutive blocks, the first that jobs with a score above
    250 reach (sf >= 126)"""
    b0 = (126 - 1) // T
    out = []
    for b in (b0, b0 + 1, b0 + 2):
        for tf in sorted({1, 25, 26, 27, T - 1, T}):
            if b * T + tf >= 126:
                out.append((b, tf))
    return out


@functools.lru_cache(maxsize=None)
def select(T):
    """-> [(p, t)]: roots of tests/tile_path_cases.py's deterministic family (4000 bases, K substitutions, short deletions near both ends) with a
    CHILD whose planned end falls at every (block, tf) of wanted(T), by the oracle's breakpoint of the root"""
    need = set(wanted(T))
    got, roots = {}, []
    kmin = 2 * (MIN_SCORE // 5) - 10  # (a child pays about half the substitutions, and its deletion)
    kmax = (2 * ((max(b for b, _ in need) + 1) * T + 2)) // 5 * 2 + 2
    for K in range(kmin, kmax + 1):
        for d0, d3 in [(a, b) for a in range(5) for b in range(5)]:
            if not need - set(got):
                return roots
            dels = (d0, 0, 0, d3)
            # (a cheap model decides which candidates the oracle is asked about: each child pays half the substitutions and its own deletion)
            guess = []
            for k, d in ((K - K // 2, d0), (K // 2, d3)):
                for s in range(5 * k + (TC._gap(O.DEFAULT_PEN, d) if d else 0) - 2, 5 * k + (TC._gap(O.DEFAULT_PEN, d) if d else 0) + 3):
                    guess.append(block_class((s + 1) // 2, s // 2, T)[:2])
            if not (set(guess) & (need - set(got))):
                continue
            p, t = TC.make_pair(K, dels, (K + d0 + d3) & 1 if any(dels) else 0)
            rc, bp, _ = O.find_breakpoint(p, t)
            if rc != 0:
                continue
            new = False
            for c in children(p, t, C_M, C_M, bp, 0):
                if not (len(c.p) and len(c.t) and c.score > MIN_SCORE):
                    continue
                sf, sr, _ = planned(c)
                cls = block_class(sf, sr, T)[:2]
                if cls in need and cls not in got:
                    got[cls] = len(roots)
                    new = True
            if new:
                roots.append((p, t))
    return roots


def covered(roots, T):
    out = set()
    for p, t in roots:
        for c in descendants(p, t):
            sf, sr, _ = planned(c)
            out.add(block_class(sf, sr, T)[:2])
    return out


@functools.lru_cache(maxsize=None)
def gap_pairs():
    """-> [(p, t)]: pairs whose root breakpoint lies inside a long deletion or insertion, so that the children end or begin in a gap component:
    3000 bases with evenly spaced substitutions and ONE long gap in the middle of them (the two directions meet inside it)"""
    out = []
    for i, (K, L, side) in enumerate([(260, 60, 0), (261, 60, 1), (130, 7, 0), (131, 7, 1), (280, 200, 0), (281, 200, 1), (150, 24, 0), (151, 3, 1)]):
        n = 3000
        p = synth.random_dna(0x9A90 + i, n)
        a = bytearray(p)
        for q in range(K):
            pos = (2 * q + 1) * n // (2 * K)
            a[pos:pos + 1] = a[pos:pos + 1].translate(TC._SUB)
        t = bytes(a)
        mid = n // 2 + 3
        if side == 0:
            t = t[:mid] + t[mid + L:]          # a deletion: the text lacks L bases
        else:
            t = t[:mid] + synth.random_dna(0x9AA0 + i, L) + t[mid:]  # an insertion
        out.append((p, t))
    return out
