"""Ends-free problems over general free lengths (shared by tests/test_oracle_wfa.py and the GPU tests; pytest does not collect it).

A WFM_MODE_ENDSFREE problem carries four independent free lengths (pbf, pef, tbf, tef): up to pbf pattern bases or tbf text bases may be
skipped before the alignment begins, up to pef / tef after it ends.  The callers of the product use two tuples only -- (plen, 0, tlen, 0)
and (0, plen, 0, tlen), the head and tail patches -- while the device implements all of them: row 0 spans [-pbf, tbf], the end tests read
pef / tef, base_columns bands a job only when pef == tef == 0.  The family here is junk(b) + core + junk(d) against
junk(a) + mutate(core) + junk(c), every pair under the tuples that put the best start and end inside, at the edge of and beyond what is
free; and the problems with an empty side, whose whole op string is one gap that both allowances of its side may shorten.

endsfree_price() reads an op string on its own (no code shared with the oracle or the device): the gap-affine two-piece price of its runs
with the free parts of the first and the last run taken off."""
import collections
import itertools
import random

from wfmash_amd import synth

DEFAULT_PEN = (5, 8, 2, 24, 1)
# default; a second affine pair within the 32-row rings; o2 + e2 = 125, the deepest scope (128-row rings); edit distance
PENS = (None, (4, 6, 2, 12, 1), (6, 10, 3, 124, 1), (1, 0, 1, 0, 1))
CORE_LENS = (0, 1, 2, 5, 60, 130, 400, 900)
RATES = (0.0, 0.05, 0.2, 0.5)
JUNK = (0, 0, 1, 3, 9, 24, 41, 70)

Case = collections.namedtuple("Case", "name p t free")  # free = (pbf, pef, tbf, tef), already within [0, len]


def clamp(free, plen, tlen):
    """what the ABI makes of a tuple: every length within [0, its sequence's length]"""
    pbf, pef, tbf, tef = free
    return (min(max(pbf, 0), plen), min(max(pef, 0), plen), min(max(tbf, 0), tlen), min(max(tef, 0), tlen))


def endsfree_price(ops, free, pen=None):
    """The cheapest price of the op string `ops` (bytes over MXID; D takes a pattern base, I a text base) as an ends-free alignment:
    mismatches at x, a gap run of L bases at min(o1 + e1 L, o2 + e2 L); up to pbf leading D or tbf leading I and up to pef trailing D or
    tef trailing I cost nothing.  The first run alone can be the skipped beginning and the last run alone the skipped end (the alignment
    begins on the pattern's or the text's first base and ends on one's last); a string of one run may use both allowances of its side."""
    x, o1, e1, o2, e2 = pen or DEFAULT_PEN
    begin = {"D": free[0], "I": free[2]}
    end = {"D": free[1], "I": free[3]}

    def gap(n):
        return 0 if n <= 0 else min(o1 + e1 * n, o2 + e2 * n)

    def paid(op, n, skip_begin, skip_end):
        if op == "M":
            return 0
        if op == "X":
            return x * n
        assert op in "DI", op
        best = None
        for fb in range(min(n, begin[op] if skip_begin else 0) + 1):
            for fe in range(min(n - fb, end[op] if skip_end else 0) + 1):
                c = gap(n - fb - fe)
                best = c if best is None or c < best else best
        return best

    runs = [(chr(op), len(list(g))) for op, g in itertools.groupby(ops)]
    return sum(paid(op, n, i == 0, i == len(runs) - 1) for i, (op, n) in enumerate(runs))


def _tuples(plen, tlen, b, d, a, c):
    """the tuples a pair runs under, clamped and without repeats, in a fixed order"""
    raw = [(0, 0, 0, 0),
           (plen, 0, tlen, 0), (0, plen, 0, tlen),  # the two patch forms
           (plen, plen, tlen, tlen),
           (b, d, a, c),  # exactly the junk
           # a few bases short of the junk at the beginning / at the end (the best start lies at the edge of row 0 or paid gap bases
           # beyond it), a few more than it, and a mixture
           (b - 3, d, a - 3, c), (b, d - 4, a, c - 4), (b + 2, d + 2, a + 2, c + 2), (b + 1, d - 1, a - 2, c + 3),
           # each of the four alone (5 where the pair has no junk there)
           (b or 5, 0, 0, 0), (0, d or 5, 0, 0), (0, 0, a or 5, 0), (0, 0, 0, c or 5),
           (3, 4, 5, 6)]
    out = []
    for f in raw:
        f = clamp(f, plen, tlen)
        if f not in out:
            out.append(f)
    return out


def pairs():
    """[(name, pattern, text, (b, d, a, c))]: every core length at every divergence, the junk lengths drawn from JUNK"""
    rng = random.Random(0xEF5)
    out = []
    for L in CORE_LENS:
        for rate in RATES:
            b, d, a, c = (rng.choice(JUNK) for _ in range(4))
            seed = 0xE0000 + 16 * L + int(rate * 100)
            core = synth.random_dna(seed, L)
            mut = synth.mutate(core, rate, seed + 1) if L else b""
            p = synth.random_dna(seed + 2, b) + core + synth.random_dna(seed + 3, d)
            t = synth.random_dna(seed + 4, a) + mut + synth.random_dna(seed + 5, c)
            out.append(("core%d_%d%%" % (L, int(rate * 100)), p, t, (b, d, a, c)))
    return out


def empty_side_cases():
    text10 = synth.random_dna(0xE51, 10)
    pat12 = synth.random_dna(0xE52, 12)
    out = []
    for f in ((0, 0, 0, 0), (0, 0, 4, 3), (0, 0, 4, 0), (0, 0, 0, 3), (0, 0, 10, 0), (0, 0, 0, 10), (0, 0, 10, 10), (0, 0, 6, 6), (0, 0, 9, 0)):
        out.append(Case("empty_x_10", b"", text10, f))
    for f in ((0, 0, 0, 0), (5, 2, 0, 0), (5, 0, 0, 0), (0, 2, 0, 0), (12, 0, 0, 0), (0, 12, 0, 0), (12, 12, 0, 0), (7, 7, 0, 0), (0, 11, 0, 0)):
        out.append(Case("12_x_empty", pat12, b"", f))
    out.append(Case("empty_x_empty", b"", b"", (0, 0, 0, 0)))
    return out


def build_cases():
    """every case of the family: the pairs under their tuples, then the empty sides"""
    out = []
    for name, p, t, (b, d, a, c) in pairs():
        for f in _tuples(len(p), len(t), b, d, a, c):
            out.append(Case(name, p, t, f))
    return out + empty_side_cases()
