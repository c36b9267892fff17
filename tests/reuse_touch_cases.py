"""Roots whose kept wavefronts touch, or just miss, the box of a level-1 child (shared by tests/test_reuse_touch_cases_cpu.py and
tests/test_reuse_touch_gpu.py).

Parent reuse ("When a kept row is the child's row") hands a BiWFA child the rows its parent kept of the
direction the two share, and is exact only while every kept cell on the child's diagonals lies strictly inside the child's box:
v < hmax_c(k) = min(tl_c, pl_c + k).  wfa_restore_kernel tests `v >= wall` over the rows and diagonals it writes and the job gives
the keep up.  Pairs that diverge uniformly never get near that test: at half a child's score its wavefront is in the middle of its box.

Where a kept cell CAN touch.  The kernel looks at the cells of the child's own row ranges (make_rng of the child's box and bound:
|k - (tl_c - pl_c)| <= sub_c - s), so a touching cell at score s is one from which the child's end is still within its bound: it lies on
a near-optimal path of the child that reaches the side of the box early and runs along it in one long gap.  That is a child whose
pattern (or text) ends where a large indel of the root begins -- the root's breakpoint fell inside that indel (a gap component) or
right behind it.  The parent's wavefront holds the gap's ray along that very row, one cell a score, for as long as the gap lasts.

The family (deterministic, no fixture): a root is  a' + m' + b'  against  a + X + m + Y + b  -- conserved pieces a, m, b
(`core` bases between them), unrelated inserts X, Y of 1500 - 3000 bases in the text (or, the pair swapped, in the pattern), 0 - 5 % of
substitutions and short indels on the conserved pieces, one or two substitutions placed d bases behind X (0 - 8, 23 - 34 one by one, 40, 56): the forward
direction passes X and runs up to that substitution, so the child's last row lies d rows beyond the gap's ray -- the distance between
the kept cells and the wall, base by base.  The length of X is set from the oracle's scores of the pieces so that the two halves cost
the same and the breakpoint falls there ("end"), or X is made to outweigh the rest so that it falls inside X ("mid": a gap component).
"exact" members are "end" members in which no cell beside the ray is extended by a chance match (see EXACT_RUN): their margin is d - 16 at
every score, so one child's keeps all touch with the furthest cell ON the wall and the next one's all stop one base short.
Every pair also comes mirrored (both sequences reversed): what child A's forward direction met is then met by child B's reverse one.
Some roots carry an N (the byte tile kernel).  Which class a child falls into is the oracle's answer alone.

Classes, per child and block length T.  A keep is taken at multiples of chunk * T scores (the cadence is whole chunks of two blocks)
from s_lo = max(1, WFM_REUSE_MIN_BLOCKS) * T rounded up to that on, and a child resumes at s_hi = reuse_resume_limit(S_c, T, 48) at
the latest.  margin(s) = min over the rows a keep holds (KEEP_ROWS: M of 26 scores, I1 / D1 of two, I2 / D2 of one) and over the
child's diagonals in its range of that row of hmax_c(k) - v:

    must touch      margin(s) <= 0 at every keep score of [s_lo, s_hi]   (so margin(s_lo) <= 0)
    must not touch  margin(s) >= 1 at every one of them                  (so margin(s_hi) >= 1)
    depends         otherwise: these only have to equal the oracle

The two end scores alone would do if the margin fell with the score.  Offsets on a diagonal never decrease, but the child's range
moves with the score (its bound lets a diagonal out), and the cells next to a gap's ray are extended by chance matches: a keep at
s_lo can touch where one at s_hi does not.  So every score a keep can be taken at is looked at; the classes are no wider for it.
"""
import collections
import functools

import numpy as np

from oracle import pyoracle as O
from wfmash_amd import synth

PEN = O.DEFAULT_PEN
FINE_MARGIN = 48          # WFM_TILE_FINE_MARGIN
MIN_BLOCKS = 8            # WFM_REUSE_MIN_BLOCKS
CHUNK = 2                 # blocks between two looks of the host: the cadence of the keeps is a multiple
SUB_SLACK = 2 * max(PEN[1], PEN[3]) + 8   # a child's bound: its score and this (push_children)
TS = (32, 100)
# (component, scores back) of the rows of a keep: keep_row of wfa_kernels.hip
KEEP = [(O.COMP["M"], b) for b in range(26)] + [(O.COMP["I1"], 0), (O.COMP["I1"], 1), (O.COMP["D1"], 0), (O.COMP["D1"], 1),
                                                (O.COMP["I2"], 0), (O.COMP["D2"], 0)]
assert len(KEEP) == 32
_SUB = bytes.maketrans(b"ACGTN", b"CGTAN")

Spec = collections.namedtuple("Spec", "kind side core gy noise d two mirror n_at seed")
Child = collections.namedtuple("Child", "dir p t par_p par_t score comp")   # all four sequences in the direction's own order (child B: reversed)
Root = collections.namedtuple("Root", "spec p t score bp children")


def resume_limit(score, T, fine_margin=FINE_MARGIN):
    """reuse_resume_limit of wfa_plan.h"""
    x = score // 2 - fine_margin
    return -1 if x < 0 else x // T * T - T


def keep_scores(score, T):
    """every score a keep the child may resume from can stand at: multiples of CHUNK * T in [s_lo, s_hi]"""
    step = CHUNK * T
    s_lo = -(-max(1, MIN_BLOCKS) * T // step) * step
    return list(range(s_lo, resume_limit(score, T) + 1, step))


def _flip(s):
    return s.translate(_SUB)


# "exact" members: X over {A, C}, the first EXACT_RUN bases of m over {G, T} -- no cell beside the gap's ray is extended by a chance match, so how far
# the kept cells reach beyond the ray is the penalties' doing alone: a deletion of L rows off the ray costs 8 + 2 L or 24 + L and moves L diagonals
# away from the child's end, which its bound (its score and 56) allows up to L = 16.  The margin is d - 16 at every score a keep can stand at.
EXACT_RUN = 48
EXACT_REACH = 16
_TO_GT = bytes.maketrans(b"ACGT", b"GTGT")
_TO_AC = bytes.maketrans(b"ACGT", b"ACAC")


def _swap_gt(s):
    return s.translate(bytes.maketrans(b"GT", b"TG"))


def _noisy(seq, rate, seed):
    return synth.mutate(seq, rate, seed) if rate > 0 else seq


@functools.lru_cache(maxsize=None)
def _score(p, t):
    rc, _, score, _ = O.align_biwfa(p, t)
    assert rc == 0
    return score


def make_pair(spec):
    """-> (pattern, text, an upper bound of the score by the pieces' own) of a Spec"""
    sd = 0x70C0000 + spec.seed * 64
    la = spec.core * 2 // 5
    a, m, b = (synth.random_dna(sd + i, n) for i, n in enumerate((la, max(100, spec.core - 2 * la), la)))
    Y = synth.random_dna(sd + 4, spec.gy)
    if spec.kind == "exact":
        m = m[:EXACT_RUN].translate(_TO_GT) + m[EXACT_RUN:]
    a2, b2 = _noisy(a, spec.noise, sd + 8), _noisy(b, spec.noise, sd + 9)
    m2 = bytearray(_noisy(m, spec.noise, sd + 10))
    if spec.kind == "mid":
        # the first gap outweighs everything behind it: the halves meet inside it
        gx = spec.gy + 2 * (_score(bytes(m2), m) + _score(b2, b)) + 1500
    else:
        # d bases of m behind X match, then one substitution (or two, three bases apart): the forward direction stops in front of it
        mt = bytearray(m)
        m2[:spec.d + 8] = mt[:spec.d + 8]
        flip = _swap_gt if spec.kind == "exact" else _flip
        m2[spec.d:spec.d + 1] = flip(bytes(mt[spec.d:spec.d + 1]))
        if spec.two:
            m2[spec.d + 3:spec.d + 4] = flip(bytes(mt[spec.d + 3:spec.d + 4]))
        # what the reverse direction pays up to there, and the forward one before X: X makes up the difference (and `two` odd points more)
        rest = _score(bytes(m2[spec.d:]), bytes(mt[spec.d:])) + PEN[3] + PEN[4] * spec.gy + _score(b2, b)
        gx = rest - PEN[3] - _score(a2, a) + (spec.seed % 3)
        if spec.mirror:
            # the mirrored pair's forward direction comes from the other side and stops behind the substitutions, if the direction that passes X pays
            # for them as well: X that much shorter
            gx -= 2 * PEN[0] * (1 + spec.two)
    X = synth.random_dna(sd + 3, gx)
    if spec.kind == "exact":
        X = X.translate(_TO_AC)
    bound = _score(a2, a) + _score(bytes(m2), m) + _score(b2, b) + 2 * PEN[3] + PEN[4] * (gx + spec.gy)
    p, t = a2 + bytes(m2) + b2, a + X + m + Y + b
    if spec.n_at:
        # one N in both, in a stretch of a the noise left alone (N matches N: no edit moves, the job runs on the byte kernels)
        at = next(i for i in range(8, spec.n_at + 1)[::-1] if p[i - 8:i + 8] == t[i - 8:i + 8])
        p, t = p[:at] + b"N" + p[at + 1:], t[:at] + b"N" + t[at + 1:]
    if spec.side == "p":
        p, t = t, p
    if spec.mirror:
        p, t = p[::-1], t[::-1]
    return p, t, bound


def specs():
    out = []

    def add(**kw):
        base = dict(kind="end", side="t", core=800, gy=2200, noise=0.02, d=0, two=0, mirror=0, n_at=0)
        base.update(kw)
        out.append(Spec(seed=len(out), **base))
    for mirror in (0, 1):
        # the child's last row d rows beyond the gap's ray: 0 - 8 (the kept cells reach up to 25 rows beyond the ray -- the child's bound has a
        # slack of 56 points, a row costs at most 5 -- so these all touch), 23 - 34 around the wall base by base, 40 and 56 well clear of it
        for i, d in enumerate((0, 1, 2, 3, 4, 5, 6, 8) + tuple(range(23, 35)) + (40, 56)):
            add(d=d, mirror=mirror, side="tp"[i % 2], core=(500, 1000, 200, 1500, 800)[i % 5], gy=(2000, 2300, 2600, 1900, 3000)[(i // 2) % 5],
                noise=(0.0, 0.02, 0.05, 0.01)[i % 4], two=int(i % 4 == 1), n_at=70 if i in (2, 11) else 0)
        add(d=0, mirror=mirror, side="p", core=3000, gy=2000, noise=0.01)
        # (more of the nearest misses: short roots have few scores a keep can stand at, and every one of them has to miss)
        for i, d in enumerate((27, 28, 29, 30)):
            add(d=d, mirror=mirror, side="tp"[i % 2], core=300, gy=1900 + 100 * i, noise=0.0)
        # the wall to the base: no chance matches beside the ray, the margin is d - 16 (mirrored: the child's last row one further)
        for i, d in enumerate((15, 16, 17, 18)):
            add(kind="exact", d=d, mirror=mirror, side="tp"[i % 2], core=(600, 400)[i // 2], gy=2000 + 150 * i, noise=0.0)
        # the breakpoint inside the gap
        for i in range(3):
            add(kind="mid", mirror=mirror, side="tp"[i % 2], core=(300, 1200, 600)[i], gy=(1500, 2000, 1700)[i], noise=(0.03, 0.0, 0.05)[i],
                n_at=60 if i == 2 else 0)
    return out


@functools.lru_cache(maxsize=None)
def roots():
    """-> [Root]: every member with the oracle's breakpoint and its two level-1 children"""
    out = []
    for spec in specs():
        p, t, bound = make_pair(spec)
        # (under a bound of the score the search leaves out the cells that cannot matter and finds the same breakpoint, field for field:
        # tests/test_oracle_wfa.py; an alignment piece by piece is such a bound)
        rc, bp, _ = O.find_breakpoint_bounded(p, t, bound)
        assert rc == 0 and bp.score <= bound, (spec, rc)
        v, h = bp.offset_forward - bp.k_forward, bp.offset_forward
        ch = (Child(0, p[:v], t[:h], p, t, bp.score_forward, bp.component),
              Child(1, p[v:][::-1], t[h:][::-1], p[::-1], t[::-1], bp.score_reverse, bp.component))
        out.append(Root(spec, p, t, bp.score, bp, ch))
    return out


def gap_open(comp):
    return 0 if comp == O.COMP["M"] else (PEN[1] if comp in (O.COMP["I1"], O.COMP["D1"]) else PEN[3])


def rng(pl, tl, sub, s):
    """rng_lo / rng_hi of wfa_rows.h"""
    return max(-pl, -s, (tl - pl) - sub + s), min(tl, s, (tl - pl) + sub - s)


def kept_cells(child, kmin, off, s):
    """the cells of the parent's rows at score s (off: forward_rows' offsets there) that a restore writes into the child's:
    [(component, back, first diagonal, offsets, walls)] over the child's range of each row"""
    pl, tl = len(child.p), len(child.t)
    out = []
    for comp, back in KEEP:
        sc = s - back
        if sc < 0:
            continue
        lo, hi = rng(pl, tl, child.score + SUB_SLACK, sc)
        if hi < lo:
            continue
        k = np.arange(lo, hi + 1)
        out.append((comp, back, lo, off[comp, back, lo - kmin:hi + 1 - kmin], np.minimum(tl, pl + k)))
    return out


def _margin(cells):
    """-> (margin, diagonals that touch): min of hmax_c(k) - v over the kept cells; a large number where no row holds a cell"""
    best, touching = 1 << 30, set()
    for _, _, lo, v, wall in cells:
        ok = v > O.ROW_NULL
        if not ok.any():
            continue
        gap = (wall - v)[ok]
        best = min(best, int(gap.min()))
        touching.update((np.nonzero(ok)[0][gap <= 0] + lo).tolist())
    return best, frozenset(touching)


@functools.lru_cache(maxsize=None)
def margins(ri, di):
    """{score: (margin, touching diagonals)} of child di of root ri at every score a keep can stand at under one of TS: one pass of the oracle over
    the parent's outer direction"""
    child = roots()[ri].children[di]
    ss = sorted({s for T in TS for s in keep_scores(child.score, T)})
    if not ss:
        return {}
    kmin, off, _ = O.forward_rows(child.par_p, child.par_t, ss)
    return {s: _margin(kept_cells(child, kmin, off[i], s)) for i, s in enumerate(ss)}


Class = collections.namedtuple("Class", "name s_lo s_hi margin_lo margin_hi least most touching")   # least, most: the margins' range over the keep scores


@functools.lru_cache(maxsize=None)
def classify(ri, di, T):
    """the class of child di of root ri under block length T; `none`: too shallow to be handed a keep at all"""
    child = roots()[ri].children[di]
    ks = keep_scores(child.score, T)
    if not ks:
        return Class("none", 0, resume_limit(child.score, T), None, None, None, None, frozenset())
    ms = [margins(ri, di)[s] for s in ks]
    vals = [m for m, _ in ms]
    name = "touch" if max(vals) <= 0 else ("clear" if min(vals) >= 1 else "depends")
    return Class(name, ks[0], ks[-1], vals[0], vals[-1], min(vals), max(vals), frozenset().union(*[t for _, t in ms]))


def side_only(ri, di, T):
    """a must-touch child that no kept cell touches on its start diagonal or on the diagonal of its corner: the side of the box alone"""
    child, c = roots()[ri].children[di], classify(ri, di, T)
    return c.name == "touch" and 0 not in c.touching and (len(child.t) - len(child.p)) not in c.touching


def table(T):
    """-> [(root index, child index, Class)] of the children that can be handed a keep"""
    return [(ri, di, classify(ri, di, T)) for ri in range(len(roots())) for di in (0, 1) if classify(ri, di, T).name != "none"]
