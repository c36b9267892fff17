"""The semantics of --transitive (include/wfmash_hip.h: wfm_trans_*) restated by brute force: the yardstick of tests/test_transitive_cpu.py
and tests/test_transitive_gpu.py.  A record is (t, q, rev, runs): t and q world positions, rev = the text is the reverse complement of the
query window, runs = [(length, op)].  A record is expanded to its aligned columns as pairs of world bases; a hull is read off the pairs.
Nothing here searches a prefix: the brute-force form shares no logic with the kernels.

The second form (Fast) is the one the driver test needs: per record the aligned runs alone as NumPy arrays, a hull by two searches among
them.  tests/test_transitive_cpu.py holds it against the brute-force form."""
import numpy as np

from tests import lift_model as LM

REVERSE, SPANS = 1, 2


def spans(runs):
    return sum(n for n, op in runs if op != "I"), sum(n for n, op in runs if op != "D")


def aligned_pairs(rec):
    """[(target world base, query world base)] of every = or X column, in column order"""
    t, q, rev, runs = rec
    cols, P, T = LM.columns(runs)
    return [(t + p, q + (T - 1 - i if rev else i)) for p, i, op in cols if op in "=X"]


def hull(rec, back, a, b):
    """hull(arc, [a, b)) or None.  back: the arc from the query window to the target"""
    pairs = [(qw, tw) if back else (tw, qw) for tw, qw in aligned_pairs(rec)]
    inside = [(s, d) for s, d in pairs if a <= s < b]  # (an aligned source base lies in the arc's source span)
    if not inside:
        return None
    first, last = min(inside), max(inside)
    return (min(first[1], last[1]), max(first[1], last[1]) + 1)


def merge(ivs):
    """the maximal intervals: abutting and overlapping ones merged, sorted"""
    out = []
    for a, b in sorted(ivs):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def step(records, R, prev=None, hull_fn=hull):
    """R_(k+1) from R_k = R (maximal intervals).  prev: R_(k-1), whose intervals are not projected again; None projects all"""
    new = list(R)
    old = set(prev) if prev is not None else set()
    for a, b in R:
        if (a, b) in old:
            continue
        for rec in records:
            for back in (False, True):
                h = hull_fn(rec, back, a, b)
                if h is not None:
                    new.append(h)
    return merge(new)


def closure(records, seed, depth, skip=True):
    """(R_depth as sorted maximal intervals, rounds run).  depth 0: to the fixed point.  A walk ends early where a round changes nothing (the
    result is the same); that round counts.  Without records no round is run."""
    R, prev, k = [tuple(seed)], None, 0
    while records and (depth == 0 or k < depth):
        new = step(records, R, prev if skip else None)
        k += 1
        if new == R:
            break
        prev, R = R, new
    return R, k


def closures(records, seeds, depth, skip=True):
    """what wfm_trans_closure returns: ([(start, end, seed)] sorted by (seed, start), [(first, count, bases)], the rounds of the call = the
    most any seed takes)"""
    ivs, per, rounds = [], [], 0
    for i, s in enumerate(seeds):
        R, k = closure(records, s, depth, skip)
        per.append((len(ivs), len(R), sum(b - a for a, b in R)))
        ivs += [(a, b, i) for a, b in R]
        rounds = max(rounds, k)
    return ivs, per, rounds


def good(rec, n_bases):
    """whether wfm_trans_add keeps the record"""
    t, q, rev, runs = rec
    if not runs or any(n == 0 for n, _ in runs):
        return False
    P, T = spans(runs)
    return P < 2 ** 32 and T < 2 ** 32 and t + P <= n_bases and q + T <= n_bases


def problems(records):
    """the records as wfm_trans_add takes them: ([(t, q, runs_off, n_runs, flags)], run words)"""
    probs, words = [], []
    for t, q, rev, runs in records:
        probs.append((t, q, len(words), len(runs), REVERSE if rev else 0))
        words += LM.words(runs)
    return probs, words


def world(tnames, tlengths, qnames, qlengths):
    """(names, lengths) of the world: the target's sequences, then the query's whose names no target has (a name twice: its first)"""
    names, lengths = [], []
    for n, ln in list(zip(tnames, tlengths)) + list(zip(qnames, qlengths)):
        if n not in names:
            names.append(n)
            lengths.append(ln)
    return names, lengths


def split(a, b, offsets):
    """[a, b) of the world cut where it crosses from one sequence into the next: [(sequence, start, end)] in the sequences' own coordinates"""
    out = []
    for s in range(len(offsets) - 1):
        lo, hi = max(a, offsets[s]), min(b, offsets[s + 1])
        if lo < hi:
            out.append((s, lo - offsets[s], hi - offsets[s]))
    return out


def file_text(names, lengths, seeds, ivs):
    """the --transitive file.  seeds: LM.parse_bed's intervals in INPUT order; ivs: [(start, end, seed)] sorted by (seed, start)"""
    off = LM.offsets(lengths)
    out = []
    for a, b, i in ivs:
        sd = seeds[i]
        for s, lo, hi in split(a, b, off):
            out.append("%s\t%d\t%d\t%s\t%s\t%d\t%d\n" % (names[s], lo, hi, sd["name"], names[sd["seq"]], sd["start"], sd["end"]))
    return "".join(out)


def parse_seeds(bed_text, names, lengths):
    """(the seeds in input order, lines skipped)"""
    kept, skipped = LM.parse_bed(bed_text, names, lengths)
    return sorted(kept, key=lambda v: v["order"]), skipped


def paf_records(paf_lines, names, lengths):
    """the records of aligned PAF lines (cg:Z: over =XID) in the world of (names, lengths)"""
    off = LM.offsets(lengths)
    out = []
    for line in paf_lines:
        f = line.rstrip("\n").split("\t")
        runs = LM.parse([v for v in f[12:] if v.startswith("cg:Z:")][0][5:])
        out.append((off[names.index(f[5])] + int(f[7]), off[names.index(f[0])] + int(f[2]), f[4] == "-", runs))
    return out


class Fast:
    """The same closure on NumPy arrays: per record the aligned runs alone (their source and destination offsets), all arcs' source
    spans in two arrays so that a round finds an interval's arcs in one comparison."""

    def __init__(self, records):
        self.arcs = []  # (world source start, world source end, ...) per arc
        S, E = [], []
        for t, q, rev, runs in records:
            n = np.array([r[0] for r in runs], dtype=np.int64)
            op = np.array(["=XID".index(r[1]) for r in runs], dtype=np.int64)
            p0 = np.concatenate(([0], np.cumsum(np.where(op != 2, n, 0))))
            t0 = np.concatenate(([0], np.cumsum(np.where(op != 3, n, 0))))
            P, T = int(p0[-1]), int(t0[-1])
            al = op <= 1
            ap, at, an = p0[:-1][al], t0[:-1][al], n[al]
            # forward: the source axis is the pattern; back: the text
            self.arcs.append(dict(s=t, slen=P, d=q, dlen=T, a0=ap, e0=ap + an, b0=at, n=an, flip_src=False, flip_dst=rev))
            self.arcs.append(dict(s=q, slen=T, d=t, dlen=P, a0=at, e0=at + an, b0=ap, n=an, flip_src=rev, flip_dst=False))
            S += [t, q]
            E += [t + P, q + T]
        self.S, self.E = np.array(S, dtype=np.int64), np.array(E, dtype=np.int64)

    def hull(self, k, a, b):
        arc = self.arcs[k]
        c0, c1 = max(a, arc["s"]) - arc["s"], min(b, arc["s"] + arc["slen"]) - arc["s"]
        if c0 >= c1 or len(arc["n"]) == 0:
            return None
        if arc["flip_src"]:
            c0, c1 = arc["slen"] - c1, arc["slen"] - c0
        a0, b0, n = arc["a0"], arc["b0"], arc["n"]
        j0 = int(np.searchsorted(arc["e0"], c0, side="right"))  # the first aligned run that ends behind c0
        j1 = int(np.searchsorted(a0, c1, side="left")) - 1   # the last aligned run that begins before c1
        if j0 > j1:
            return None
        s0, s1 = max(c0, int(a0[j0])), min(c1, int(a0[j1] + n[j1]))
        d0, d1 = int(b0[j0]) + s0 - int(a0[j0]), int(b0[j1]) + s1 - int(a0[j1])
        if arc["flip_dst"]:
            d0, d1 = arc["dlen"] - d1, arc["dlen"] - d0
        return (arc["d"] + d0, arc["d"] + d1)

    def step(self, R, prev):
        new = list(R)
        old = set(prev) if prev is not None else set()
        for a, b in R:
            if (a, b) in old:
                continue
            for k in np.nonzero((self.S < b) & (self.E > a))[0]:
                h = self.hull(int(k), a, b)
                if h is not None:
                    new.append(h)
        return merge(new)

    def closure(self, seed, depth):
        R, prev, k = [tuple(seed)], None, 0
        while self.arcs and (depth == 0 or k < depth):
            new = self.step(R, prev)
            k += 1
            if new == R:
                break
            prev, R = R, new
        return R, k

    def closures(self, seeds, depth):
        ivs, per, rounds = [], [], 0
        for i, s in enumerate(seeds):
            R, k = self.closure(s, depth)
            per.append((len(ivs), len(R), sum(b - a for a, b in R)))
            ivs += [(a, b, i) for a, b in R]
            rounds = max(rounds, k)
        return ivs, per, rounds
