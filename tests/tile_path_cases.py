"""Pairs whose BiWFA directions meet at chosen places of a tile block (shared by tests/test_tile_path_cases_cpu.py and
tests/test_tile_paths_gpu.py).

The tile phase of the align path (run_tiled_phase, wfa_tile_advance_kernel, wfa_tile2_kernel) advances a job in blocks of T scores and
branches on where the job's two directions meet relative to a block: the block's index b, the steps tf / tr the forward / reverse
direction have taken into it, tf = 1 with tr = 0, tf = T, min(tf, tr) < 26.  The oracle reports that point (pyoracle.meet_point:
(sf, sr, last_fwd) where the first loop of the breakpoint search ends), and

    b = (sf - 1) // T,  tf = sf - b * T,  tr = sr - b * T.

The family is deterministic and needs no fixture: a random pattern of 4000 bases, the text a copy with K evenly spaced substitutions
and up to four short deletions (1 - 4 bases) at fixed sites near 10 % and 90 % of the length -- taken from the text (tl < pl) or from
the pattern (tl > pl).  Every event has to be paid by the direction that passes it, so a cheap model (predict) says where a candidate
will meet; it only decides which candidates the oracle is asked about.  What goes into a selection is the oracle's answer alone.
"""
import collections
import functools

import numpy as np

from oracle import pyoracle as O
from wfmash_amd import synth

N = 4000
SEED = 0x711E
ALT_PEN = (4, 6, 2, 12, 1)
# (per mille of the length, offset): where deletions go.  The issue's family has the first and the last site; the two inner ones
# were added because T = 32 needs meeting scores (33, 34, 59 ...) that one deletion per side cannot make of 5 K + {10, 12, 14, 16}
SITES = ((100, 7), (150, 11), (850, 5), (900, 3))
_SUB = bytes.maketrans(b"ACGT", b"CGTA")

Case = collections.namedtuple("Case", "K dels side p t sf sr last_fwd")  # dels: one length per site of SITES (0: none)


def edges(T):
    """the (tf, tr) every block of 1 .. 3 must be met at: first step, around the 26 rows phase 2 reads behind a run, last step"""
    return [(1, 0), (1, 1), (2, 1), (25, 24), (25, 25), (26, 25), (26, 26), (27, 26), (27, 27),
            (T - 1, T - 2), (T - 1, T - 1), (T, T - 1), (T, T)]


# block 0 (prev_ok false: no block before it to run again): what the family reaches -- the cheapest member costs 5 a direction
BLOCK0 = {100: [(25, 24), (25, 25), (26, 25), (26, 26), (27, 26), (27, 27), (99, 98), (99, 99), (100, 99), (100, 100)],
          32: [(25, 24), (25, 25), (26, 25), (26, 26), (27, 26), (27, 27), (31, 30), (31, 31), (32, 31), (32, 32)]}


PLAIN_K = {100: (10, 41, 42, 77, 120, 158), 32: (10, 13, 20, 41, 42, 50)}


def required(T, pen=None):
    """the (b, tf, tr) classes a selection must hold.  Under ALT_PEN every event costs an even number (4; 8, 10, 12, 14 for a gap of
    1 .. 4), so a direction's reach only grows at even scores and the loop can only end with tf even: the odd classes do not exist there"""
    req = [(0,) + e for e in BLOCK0[T]] + [(b,) + e for b in (1, 2, 3) for e in edges(T)]
    if pen is not None and tuple(pen) == ALT_PEN:
        req = [c for c in req if c[1] % 2 == 0]
    return req


def classify(sf, sr, T):
    b = (sf - 1) // T
    return b, sf - b * T, sr - b * T


@functools.lru_cache(maxsize=None)
def pattern():
    return synth.random_dna(SEED, N)


def sub_positions(K):
    return [(2 * i + 1) * N // (2 * K) for i in range(K)]


def make_pair(K, dels, side):
    """-> (pattern, text): K substitutions in the text; the deletions cut from the text (side 0) or from the pattern (side 1)"""
    p = pattern()
    a = bytearray(p)
    for pos in sub_positions(K):
        a[pos:pos + 1] = a[pos:pos + 1].translate(_SUB)
    t = bytes(a)
    cuts = sorted(((N * pm // 1000 + off, d) for (pm, off), d in zip(SITES, dels) if d), reverse=True)

    def cut(s):
        for pos, d in cuts:
            s = s[:pos] + s[pos + d:]
        return s
    return (p, cut(t)) if side == 0 else (cut(p), t)


def n_twin(case):
    """the same pair with one base replaced by N at the same place in pattern and text, ahead of the first deletion site and at least
    8 bases from a substitution: N matches N, every edit stays where it was -- and the job runs on the byte kernels"""
    subs = sub_positions(case.K)
    pos = 200
    while any(abs(pos - s) < 8 for s in subs):
        pos += 9
    assert pos < N * SITES[0][0] // 1000
    assert case.p[pos] == case.t[pos]
    return case.p[:pos] + b"N" + case.p[pos + 1:], case.t[:pos] + b"N" + case.t[pos + 1:]


def _gap(pen, d):
    return min(pen[1] + d * pen[2], pen[3] + d * pen[4])


@functools.lru_cache(maxsize=None)
def _sub_array(K):
    return np.array(sub_positions(K))


def predict(K, dels, pen):
    """(sf, sr) a candidate is expected to meet at: the forward direction pays the events from the left, the reverse one from the right,
    and the loop ends at the first alternating step at which the two have paid all of them between them"""
    at = [(N * pm // 1000 + off, _gap(pen, d)) for (pm, off), d in zip(SITES, dels) if d]
    c = np.full(K, pen[0])
    if at:
        c = np.insert(c, np.searchsorted(_sub_array(K), [a[0] for a in at]), [a[1] for a in at])
    f = np.concatenate(([0], np.cumsum(c)))                      # f[j]: the forward direction has passed j events
    r = np.concatenate(([0], np.cumsum(c[::-1])))[::-1]          # r[j]: the reverse one the other E - j
    fw = f > r
    sf, sr = np.where(fw, f, r), np.where(fw, f - 1, r)
    i = int(np.argmin(sf + sr))
    return int(sf[i]), int(sr[i])


def _candidates(kmin, kmax, inner):
    """(K, dels, side) in a fixed order; `inner`: deletions at the two inner sites as well"""
    lens = range(5)
    for K in range(kmin, kmax + 1):
        for d0 in lens:
            for d3 in lens:
                for d1 in (lens if inner else (0,)):
                    for d2 in ((0, d1) if inner else (0,)):  # (the inner sites: one of them, or both alike -- enough for every class)
                        if d2 and not d1:
                            continue
                        dels = (d0, d1, d2, d3)
                        yield K, dels, (K + d0 + d3 + d1) & 1 if any(dels) else 0


def _ask(cand, pen):
    K, dels, side = cand
    p, t = make_pair(K, dels, side)
    sf, sr, lf = O.meet_point(p, t, pen)
    return Case(K, dels, side, p, t, sf, sr, lf)


@functools.lru_cache(maxsize=None)
def select(T, pen=None, spread=48, tries=24):
    """-> [Case]: one pair for every class of required(T, pen) the family reaches, then `spread` more at other offsets of blocks 0 .. 3.
    Which classes are in it is for the caller to check (covered)."""
    pn = tuple(pen or O.DEFAULT_PEN)
    kmax = (8 * T + 40) // pn[0] + 2            # (a direction pays about half the events: a deeper candidate meets beyond block 3)
    by_pred = collections.defaultdict(list)
    for cand in _candidates(1, min(kmax, 210), inner=True):
        sf, sr = predict(cand[0], cand[1], pn)
        if sf <= 4 * T:
            by_pred[classify(sf, sr, T)].append(cand)
    got, asked = {}, set()

    def ask(cand):
        if cand in asked:
            return
        asked.add(cand)
        c = _ask(cand, pn)
        if c.sf > 0:
            got.setdefault(classify(c.sf, c.sr, T), c)
    for cls in required(T, pen):
        for cand in by_pred.get(cls, [])[:tries]:
            if cls in got:
                break
            ask(cand)
    out = [got[c] for c in required(T, pen) if c in got]
    # other offsets: every seventh step of the blocks (T = 32: every third), both parities of the exit, alternating sides -- again by the oracle's answer
    want = [(b, tf, tf - lf) for b in range(4) for tf in range(5, T, 7 if T >= 64 else 3) for lf in (0, 1)]
    want = [w for w in want if w not in set(required(T, pen))]
    step = max(1, len(want) // spread)
    extra = {}
    for w in want[::step]:
        for cand in by_pred.get(w, [])[:2]:
            c = None
            if cand not in asked:
                asked.add(cand)
                c = _ask(cand, pn)
            if c is not None and c.sf > 0:
                cl = classify(c.sf, c.sr, T)
                if cl not in set(required(T, pen)) and cl[0] <= 3 and cl not in extra:
                    extra[cl] = c
                    break
    out += [extra[k] for k in sorted(extra)]
    # and the plain members, substitutions alone (pl = tl; 41 and 42 are the pair tests/test_oracle_wfa.py pins by hand)
    have = {(c.K, c.dels) for c in out}
    for K in PLAIN_K[T]:
        if (K, (0, 0, 0, 0)) not in have:
            out.append(_ask((K, (0, 0, 0, 0), 0), pn))
    return out


def covered(cases, T):
    return {classify(c.sf, c.sr, T) for c in cases}


@functools.lru_cache(maxsize=None)
def wide_set():
    """-> [(pattern, text, sf)]: the halo paths.  Sixteen pairs of 1500 - 3000 bases mutated at 20 - 30 %: deep jobs whose rows cross
    threads * 2 diagonals on the way, so they go from one tile without a halo to several with halos (WFM_TILE_THREADS=256: the host's
    range of a block that ends at score s is 2 s + 1 diagonals, beyond 512 from the block of scores 201 .. 300 on, at T = 100).  Pairs
    that long and that far apart meet thousands of scores later; the ones that meet IN that first block of several tiles are the same
    generator on 300 - 520 bases (scores of 400 - 600), picked by the oracle's sf."""
    out = []
    for i in range(16):
        n = 1500 + (i * 1500) // 15
        p = synth.random_dna(0x71D0 + i, n)
        t = synth.mutate(p, 0.20 + 0.10 * (i % 5) / 4, 0x71D00 + i)
        out.append((p, t, O.meet_point(p, t)[0]))
    first = []
    for i in range(40):
        n = 300 + 11 * (i % 21)
        p = synth.random_dna(0x71E0 + i, n)
        t = synth.mutate(p, 0.20 + 0.10 * (i % 3) / 2, 0x71E00 + i)
        sf = O.meet_point(p, t)[0]
        if 200 < sf <= 300 and min(len(p), 300) + min(len(t), 300) + 1 > 312:  # (its own rows there are wider than one core of Wt - 2 T = 312 diagonals)
            first.append((p, t, sf))
        if len(first) == 6:
            break
    return out + first
