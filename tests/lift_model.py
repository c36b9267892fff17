"""The semantics of --lift (include/wfmash_hip.h: wfm_liftset_*, wfm_lift_runs; include/wfmash_host.h: wfmh_set_lift) restated in plain
Python by brute force: the yardstick of tests/test_lift_cpu.py and tests/test_lift_gpu.py.

The pattern is the target, the text the query as aligned.  A run list is expanded to one (p, t, op) per column; a lift is read off the
columns.  Nothing here searches a prefix: the model shares no logic with the kernels.

With an interval clipped to the problem's pattern span, [c0, c1), and a pattern base called aligned where an = or X column holds it:
p0 = the first aligned pattern base >= c0, p1 = one past the last aligned pattern base < c1, t0 / t1 - 1 = the text bases opposite p0 /
p1 - 1, eq / x = the = / X columns between them.  No aligned base in [c0, c1): p0 = p1 = c0, t0 = t1 = the text index reached at c0."""
import re

OPS = "=XID"
LIFT_SPANS = 2


def parse(cigar):
    """'3=2D3=' -> [(3, '='), (2, 'D'), (3, '=')]"""
    runs = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cigar)]
    assert "".join("%d%s" % r for r in runs) == cigar, cigar
    return runs


def words(runs):
    """the run words of the device: (length << 2) | op"""
    return [(n << 2) | OPS.index(op) for n, op in runs]


def columns(runs):
    """[(p, t, op)] per column: the pattern and text indices the column stands at (an I column holds no pattern base, a D column no
    text base: the index is the one reached so far), and (plen, tlen)"""
    cols, p, t = [], 0, 0
    for n, op in runs:
        for _ in range(n):
            cols.append((p, t, op))
            if op != "I":
                p += 1
            if op != "D":
                t += 1
    return cols, p, t


def by_base(cols):
    """at[p] = (t, op) of the column that holds pattern base p (op is =, X or D)"""
    return [(t, op) for p, t, op in cols if op != "I"]


def lift_columns(at, c0, c1):
    """(p0, p1, t0, t1, eq, x) of the clipped interval [c0, c1), c0 < c1 <= plen: every pattern base of it is looked at"""
    inside = [(p, at[p][0], at[p][1]) for p in range(c0, c1) if at[p][1] in "=X"]
    if not inside:
        return (c0, c0, at[c0][0], at[c0][0], 0, 0)
    first, last = inside[0], inside[-1]
    return (first[0], last[0] + 1, first[1], last[1] + 1, sum(1 for c in inside if c[2] == "="), sum(1 for c in inside if c[2] == "X"))


def lift_problems(problems, intervals, n_bases):
    """what wfm_lift_runs returns: ([(problem, interval, p0, p1, t0, t1, eq, x)], [(flags, n_runs, first, count)]).
    problems = [(base, [(length, op)])]; intervals = [(start, end)] sorted, in global coordinates"""
    lifts, per = [], []
    for k, (base, runs) in enumerate(problems):
        if not runs or any(n == 0 for n, _ in runs):
            per.append((LIFT_SPANS, len(runs), len(lifts), 0))
            continue
        cols, plen, tlen = columns(runs)
        if base > n_bases or base + plen > n_bases:
            per.append((LIFT_SPANS, len(runs), len(lifts), 0))
            continue
        at = by_base(cols)
        assert len(at) == plen and [p for p, _, op in cols if op != "I"] == list(range(plen))
        first = len(lifts)
        for i, (s, e) in enumerate(intervals):
            lo, hi = max(s, base), min(e, base + plen)
            if lo < hi:
                lifts.append((k, i) + lift_columns(at, lo - base, hi - base))
        per.append((0, len(runs), first, len(lifts) - first))
    return lifts, per


def offsets(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return out


def parse_bed(text, names, lengths):
    """(intervals sorted by (global start, global end, input order), lines skipped).  An interval is a dict with seq, start, end, name,
    order (its number among the lines kept), gstart, gend.  Tab-separated, three columns at least, column 4 the name ('.' without one).
    Skipped and counted: blank lines, lines that begin with '#', 'track' or 'browser' lines, fewer than three columns, a start or end that
    is not a plain decimal of at most 18 digits, a sequence the target does not have, start >= end, end beyond the sequence."""
    off = offsets(lengths)
    kept, skipped = [], 0
    lines = text.split("\n")
    if lines[-1] == "":
        lines.pop()  # (what follows the last newline is no line)
    for line in lines:
        if line.endswith("\r"):
            line = line[:-1]
        f = line.split("\t")
        head = re.split(r"[ \t]", line, 1)[0]
        ok = line.strip(" \t") != "" and not line.startswith("#") and head not in ("track", "browser") and len(f) >= 3
        ok = ok and all(re.fullmatch(r"[0-9]{1,18}", v) for v in f[1:3]) and f[0] in names
        if ok:
            c, a, b = names.index(f[0]), int(f[1]), int(f[2])
            ok = a < b <= lengths[c]
        if not ok:
            skipped += 1
            continue
        kept.append(dict(seq=c, start=a, end=b, name=f[3] if len(f) > 3 and f[3] else ".", order=len(kept), gstart=off[c] + a, gend=off[c] + b))
    kept.sort(key=lambda v: (v["gstart"], v["gend"], v["order"]))
    return kept, skipped


def bed_dump(intervals, skipped):
    """the head of the test hook's answer: what the parser made of the BED"""
    out = ["#skipped\t%d\n" % skipped]
    out += ["#iv\t%d\t%d\t%d\t%s\t%d\t%d\t%d\n" % (v["seq"], v["start"], v["end"], v["name"], v["order"], v["gstart"], v["gend"]) for v in intervals]
    return "".join(out)


def lift_line(rec, iv, names, lift):
    """one line of the lift file.  rec = (qname, qs, qe, strand, tname, ts): the record's query window, strand and target start as its PAF
    line has them; lift = (p0, p1, t0, t1, eq, x)"""
    qname, qs, qe, strand, tname, ts = rec
    p0, p1, t0, t1, eq, x = lift
    a, b = (qs + t0, qs + t1) if strand == "+" else (qe - t1, qe - t0)
    return "%s\t%d\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (qname, a, b, iv["name"], strand, tname, ts + p0, ts + p1, iv["start"], iv["end"],
                                                                     eq, x, (t1 - t0) - (eq + x), (p1 - p0) - (eq + x))


def lift_paf(paf_lines, bed_text, names, lengths):
    """the lift file of aligned PAF lines (cg:Z: over =XID), and (records lifted, lines, empty lifts, BED lines skipped)"""
    intervals, skipped = parse_bed(bed_text, names, lengths)
    off = offsets(lengths)
    out, empty, records = [], 0, 0
    for line in paf_lines:
        f = line.rstrip("\n").split("\t")
        runs = parse([v for v in f[12:] if v.startswith("cg:Z:")][0][5:])
        c = names.index(f[5])
        rec = (f[0], int(f[2]), int(f[3]), f[4], f[5], int(f[7]))
        lifts, per = lift_problems([(off[c] + rec[5], runs)], [(v["gstart"], v["gend"]) for v in intervals], off[-1])
        assert per[0][0] == 0
        records += 1
        for lf in lifts:
            out.append(lift_line(rec, intervals[lf[1]], names, lf[2:]))
            empty += lf[6] + lf[7] == 0
    return "".join(out), (records, len(out), empty, skipped)
