"""The semantics of --coverage (include/wfmash_hip.h: wfm_coverage_*; include/wfmash_host.h: wfmh_set_coverage) restated in numpy: the
yardstick of tests/test_coverage_cpu.py and tests/test_coverage_gpu.py.

depth(c, x) = the number of records with an = or X base at position x of target sequence c.  D bases do not count, I runs advance
nothing.  The file is plain bedGraph without a track line: per sequence, in index order, the maximal intervals of constant depth tiling
[0, length) exactly, depth 0 included; a sequence of length 0 has no line."""
import re

import numpy as np

OPS = "=XID"


def parse(cigar):
    """'3=2D3=' -> [(3, '='), (2, 'D'), (3, '=')]; S and H clips of a SAM CIGAR are dropped (they take no target base)"""
    runs = [(int(n), op) for n, op in re.findall(r"(\d+)([=XIDSH])", cigar)]
    assert "".join("%d%s" % r for r in runs) == cigar, cigar
    return [(n, op) for n, op in runs if op in OPS]


def words(runs):
    """the run words of the device: (length << 2) | op"""
    return [(n << 2) | OPS.index(op) for n, op in runs]


def diff_of(problems, n_bases):
    """the difference array, n_bases + 1 words, of problems = [(base, runs)]: +1 where an aligned base follows one that is not, -1 behind
    the last of a stretch -- taken per run here, which sums to the same array"""
    d = np.zeros(n_bases + 1, dtype=np.int64)
    for base, runs in problems:
        p, plus, minus = base, [], []
        for n, op in runs:
            if op in "=X":
                plus.append(p)
                minus.append(p + n)
            if op != "I":
                p += n
        np.add.at(d, plus, 1)
        np.add.at(d, minus, -1)
    return d


def depth_of(problems, n_bases):
    """dense depth over the concatenation: problems = [(base, [(length, op)])], base = the global index of the first pattern base"""
    return np.cumsum(diff_of(problems, n_bases))[:n_bases]


def entries_of(problems, n_bases):
    """what wfm_coverage_export returns: [(pos, delta)] of the non-zero words"""
    d = diff_of(problems, n_bases)
    nz = np.flatnonzero(d)
    return [(int(p), int(d[p])) for p in nz]


def intervals_of(problems, n_bases):
    """what wfm_coverage_intervals returns: ([(start, depth)], (covered bases, sum of depth, max depth))"""
    depth = depth_of(problems, n_bases)
    if n_bases == 0:
        return [(0, 0)], (0, 0, 0)
    starts = np.concatenate(([0], np.flatnonzero(np.diff(depth)) + 1))
    return [(int(s), int(depth[s])) for s in starts], (int(np.count_nonzero(depth)), int(depth.sum()), int(depth.max()))


def offsets(lengths):
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64)))).astype(np.int64)


def problems_of_paf(lines, names, lengths):
    """aligned PAF lines (cg:Z: over =XID) as problems over the concatenation; returns (problems, total of the = and X run lengths)"""
    off, out, aligned = offsets(lengths), [], 0
    for line in lines:
        f = line.split("\t")
        runs = parse([x for x in f[12:] if x.startswith("cg:Z:")][0][5:])
        c = names.index(f[5])
        assert int(f[6]) == lengths[c]
        assert sum(n for n, op in runs if op != "I") == int(f[8]) - int(f[7])
        out.append((int(off[c]) + int(f[7]), runs))
        aligned += sum(n for n, op in runs if op in "=X")
    return out, aligned


def problems_of_sam(lines, names, lengths):
    """the same for SAM records (RNAME, 1-based POS, an =/X CIGAR)"""
    off, out, aligned = offsets(lengths), [], 0
    for line in lines:
        if line.startswith("@"):
            continue
        f = line.split("\t")
        runs = parse(f[5])
        out.append((int(off[names.index(f[2])]) + int(f[3]) - 1, runs))
        aligned += sum(n for n, op in runs if op in "=X")
    return out, aligned


def bedgraph(names, lengths, depth):
    """the file: depth is the dense depth over the concatenation of the sequences"""
    off, out = offsets(lengths), []
    for c, name in enumerate(names):
        d = np.asarray(depth[off[c]:off[c + 1]])
        if len(d) == 0:
            continue
        starts = np.concatenate(([0], np.flatnonzero(np.diff(d)) + 1, [len(d)]))
        out += ["%s\t%d\t%d\t%d\n" % (name, a, b, d[a]) for a, b in zip(starts[:-1], starts[1:])]
    return "".join(out)


def parse_bedgraph(text, names, lengths):
    """a bedGraph back into dense depth over the concatenation, and its number of lines.  Asserts the form on the way: four fields, the
    sequences in index order, per sequence intervals that tile [0, length) exactly, are not empty and differ in depth from their
    neighbours; a sequence of length 0 has no line, every other at least one"""
    off = offsets(lengths)
    depth = np.full(int(off[-1]), -1, dtype=np.int64)
    at = {}    # per sequence: where its next interval must begin
    last = {}  # ... and the depth of the one before
    order = []
    lines = text.splitlines(keepends=True)
    for line in lines:
        assert line.endswith("\n")
        f = line[:-1].split("\t")
        assert len(f) == 4, line
        name, a, b, d = f[0], int(f[1]), int(f[2]), int(f[3])
        c = names.index(name)
        if name not in at:
            assert not order or names.index(order[-1]) < c, "sequences out of index order"
            order.append(name)
            at[name] = 0
        else:
            assert order[-1] == name, "a sequence's lines are not together"
            assert last[name] != d, "neighbours of the same depth: the interval is not maximal"
        assert a == at[name] and a < b <= lengths[c] and d >= 0, line
        depth[off[c] + a:off[c] + b] = d
        at[name], last[name] = b, d
    for c, name in enumerate(names):
        if lengths[c] == 0:
            assert name not in at
        else:
            assert at.get(name) == lengths[c], "sequence %s is not tiled to its end" % name
    return depth, len(lines)
