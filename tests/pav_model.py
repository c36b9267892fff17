"""The semantics of --pav (include/wfmash_hip.h: wfm_pav_*; include/wfmash_host.h: wfmh_set_pav) restated by brute force: the yardstick
of tests/test_pav_cpu.py and tests/test_pav_gpu.py.

pav(j, g) = the number of bases of interval j that lie under an = or X base of at least one record of group g.  D bases do not count, I
runs advance nothing.  One boolean array per group over the concatenation of the target's sequences; a cell is sum(mask[g, a:b])."""
import numpy as np

from tests import coverage_model as V

parse, words, offsets = V.parse, V.words, V.offsets


def group_key(name, delim="#"):
    """the part before the LAST delimiter, else the whole name"""
    at = name.rfind(delim)
    return name if at < 0 else name[:at]


def columns(names, delim="#"):
    """the distinct keys of ALL the names, sorted bytewise"""
    return sorted({group_key(n, delim) for n in names}, key=lambda s: s.encode())


def mask_of(problems, n_bases, n_groups):
    """problems = [(base, runs, group)]"""
    m = np.zeros((n_groups, n_bases), dtype=bool)
    for base, runs, g in problems:
        p = base
        for n, op in runs:
            if op in "=X":
                m[g, p:p + n] = True
            if op != "I":
                p += n
    return m


def union_of(mask):
    """what wfm_pav_export returns: [(start, length, group)], the maximal runs of true per group, sorted by (group, start)"""
    out = []
    for g in range(mask.shape[0]):
        d = np.diff(np.concatenate(([0], mask[g].astype(np.int8), [0])))
        for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)):
            out.append((int(a), int(b - a), g))
    return out


def matrix_of(mask, intervals):
    """what wfm_pav_matrix returns: [interval][group]"""
    return [[int(mask[g, a:b].sum()) for g in range(mask.shape[0])] for a, b in intervals]


def segments_of(problems):
    """how many segments wfm_pav_add appends: one per maximal stretch of =/X runs"""
    n = 0
    for _, runs, _ in problems:
        prev = "D"
        for _, op in runs:
            n += op in "=X" and prev not in "=X"
            prev = op
    return n


def windows(names, lengths, size):
    """--pav-window: [(seq, start, end)] tiling every sequence in index order, the last window shorter"""
    return [(c, a, min(a + size, lengths[c])) for c in range(len(names)) for a in range(0, lengths[c], size)]


def header(cols):
    return "\t".join(["#tname", "tstart", "tend", "name", "len"] + list(cols)) + "\n"


def row(tname, a, b, name, cells):
    return "\t".join([tname, str(a), str(b), name, str(b - a)] + [str(int(c)) for c in cells]) + "\n"


def problems_of_paf(lines, tnames, tlengths, cols, delim="#"):
    """aligned PAF lines as problems [(base, runs, group)] over the concatenation of the target's sequences"""
    plain, _ = V.problems_of_paf(lines, tnames, tlengths)
    return [(base, runs, cols.index(group_key(line.split("\t")[0], delim))) for (base, runs), line in zip(plain, lines)]


def file_of(tnames, tlengths, cols, intervals, problems):
    """the --pav file: intervals = [(seq, start, end, name)] in the file's order"""
    off = offsets(tlengths)
    mask = mask_of(problems, int(off[-1]), len(cols))
    cells = matrix_of(mask, [(int(off[c]) + a, int(off[c]) + b) for c, a, b, _ in intervals])
    return header(cols) + "".join(row(tnames[c], a, b, name, cells[j]) for j, (c, a, b, name) in enumerate(intervals))
