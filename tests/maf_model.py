"""The rule of --maf (include/wfmash_hip.h: wfm_maf_rows; wfmash_amd/host/maf_text.hpp) restated in plain Python by brute force, and its
inverse: the yardstick of tests/test_maf_cpu.py and tests/test_maf_gpu.py.

Runs are (length, op) with op one of 'M', 'X', 'I', 'D' ('=' reads as 'M': left_align_model's convention); P is the pattern (target), T
the text (query AS ALIGNED: the reverse complement of the query window for a '-' record), both bytes.  A run list is expanded to one op
per column; breaks and blocks are ranges of that column string, and the two rows of ALL columns are laid down run by run and cut at those
ranges: nothing here takes a prefix or searches one, so the model shares no logic with the kernels.

Every column yields one byte in row P and one in row T: the base, or '-' in row P under an I column and in row T under a D column.  A gap
stretch is a maximal sequence of I / D columns.  With split = 0 a problem is one block; with split >= 1 a gap stretch of split or more
columns is a break: its columns are not written, the block before it ends and the next begins behind it."""
import re

from oracle import wflign_host as W

NOT_DONE, SPANS = 1, 2
HEADER = b"##maf version=1\n"


def columns(runs):
    """one op per column"""
    return "".join(op * n for n, op in runs)


def _pieces(runs, split):
    """(the column string, [(first column, end column)] of the blocks: the maximal column ranges between breaks)"""
    ops = columns(runs)
    breaks = [m.span() for m in re.finditer(r"[ID]+", ops) if split >= 1 and m.end() - m.start() >= split]
    pieces, at = [], 0
    for a, b in breaks + [(len(ops), len(ops))]:
        if a > at:
            pieces.append((at, a))
        at = b
    return ops, pieces


def blocks_of(runs, split=0):
    """[(p, t, psize, tsize, cols, eq, x)] of a run list: where each block begins in P and T, the non-gap bytes of its two rows, its
    columns and its = and X columns"""
    ops, pieces = _pieces(runs, split)
    out = []
    p = t = at = 0
    for a, b in pieces:
        skipped, inside = ops[at:a], ops[a:b]  # (the break before the block, then the block)
        p += len(skipped) - skipped.count("I")
        t += len(skipped) - skipped.count("D")
        out.append((p, t, len(inside) - inside.count("I"), len(inside) - inside.count("D"), len(inside), inside.count("M"), inside.count("X")))
        p += out[-1][2]
        t += out[-1][3]
        at = b
    return out


def rows_of(P, T, runs, split=0):
    """([(row P, row T)] one pair per block, in block order) of a run list over its bases"""
    _, pieces = _pieces(runs, split)
    pi = ti = 0
    rp, rt = bytearray(), bytearray()
    for n, op in runs:  # the two rows of ALL columns, cut below
        rp += b"-" * n if op == "I" else P[pi:pi + n]
        rt += b"-" * n if op == "D" else T[ti:ti + n]
        pi += n if op != "I" else 0
        ti += n if op != "D" else 0
    assert len(rp) == len(rt) == sum(n for n, _ in runs)
    return [(bytes(rp[a:b]), bytes(rt[a:b])) for a, b in pieces]


def refused(P, T, runs):
    """what the device flags WFM_MAF_SPANS: an empty run, two neighbours with one op, totals other than len(P) x len(T)"""
    return (any(n == 0 for n, _ in runs) or any(a[1] == b[1] for a, b in zip(runs, runs[1:]))
            or sum(n for n, op in runs if op != "I") != len(P) or sum(n for n, op in runs if op != "D") != len(T))


def call_of(cases, split=0):
    """what wfm_maf_rows returns for [(P, T, runs)]: (blocks [(off, problem, p, t, psize, tsize, cols, eq, x)], rows, per [(flags, n_runs,
    first, count)]).  A problem without runs is NOT_DONE."""
    blocks, rows, per = [], bytearray(), []
    for i, (P, T, runs) in enumerate(cases):
        if not runs:
            per.append((NOT_DONE, 0, len(blocks), 0))
            continue
        if refused(P, T, runs):
            per.append((SPANS, len(runs), len(blocks), 0))
            continue
        shape = blocks_of(runs, split)
        per.append((0, len(runs), len(blocks), len(shape)))
        for b, (rp, rt) in zip(shape, rows_of(P, T, runs, split)):
            blocks.append((len(rows), i) + b)
            rows += rp + rt
    return blocks, bytes(rows), per


def block_text(tname, tstart, psize, tsize_total, qname, qstart, tsize, strand, qsize_total, eq, row_p, row_t):
    """one paragraph of the file: single spaces, no padding"""
    return (b"a score=%d\ns %s %d %d + %d %s\ns %s %d %d %s %d %s\n\n"
            % (eq, tname.encode(), tstart, psize, tsize_total, row_p, qname.encode(), qstart, tsize, strand.encode(), qsize_total, row_t))


def record_bases(seqs, r):
    """(P, T) of a record: target [ts, te), query [qs, qe) strand-adjusted, normalised as the driver's windows are"""
    q = W.upper_valid_dna(seqs[r["qname"]][r["qs"]:r["qe"]])
    if r["strand"] == "-":
        q = W.revcomp(q)
    return W.upper_valid_dna(seqs[r["tname"]][r["ts"]:r["te"]]), q


def maf_text(records, seqs, split=0, header=True):
    """the MAF file's bytes from PAF fields and the FASTA alone.  A record is a dict with qname, qsize, qs, qe, strand, tname, tsize, ts,
    te as its PAF line has them (forward coordinates, half-open) and runs, the line's cg:Z:; seqs: name -> bases.  The target is always +
    and starts at ts + p; the query starts at qs + t on +, and on - at qsize - qe + t: the start on the reverse-complemented source, whose
    strand row T is."""
    out = [HEADER] if header else []
    for r in records:
        P, T = record_bases(seqs, r)
        assert not refused(P, T, r["runs"]), r
        for (p, t, psize, tsize, _, eq, _), (rp, rt) in zip(blocks_of(r["runs"], split), rows_of(P, T, r["runs"], split)):
            qstart = (r["qsize"] - r["qe"] if r["strand"] == "-" else r["qs"]) + t
            out.append(block_text(r["tname"], r["ts"] + p, psize, r["tsize"], r["qname"], qstart, tsize, r["strand"], r["qsize"], eq, rp, rt))
    return b"".join(out)


def parse_maf(text):
    """[block] of a MAF file: a dict with score, tname, tstart, psize, tstrand, tsize, row_p, qname, qstart, qsize_row (the row's non-gap
    bytes), qstrand, qsize, row_t.  Splits on whitespace, as MAF readers do."""
    if isinstance(text, bytes):
        text = text.decode()
    assert text.startswith(HEADER.decode())
    blocks = []
    for para in text[len(HEADER):].split("\n\n"):
        lines = [ln for ln in para.split("\n") if ln]
        if not lines:
            continue
        assert len(lines) == 3 and re.fullmatch(r"a score=\d+", lines[0]), para[:200]
        a, b = lines[1].split(), lines[2].split()
        assert a[0] == "s" and b[0] == "s" and len(a) == 7 and len(b) == 7, para[:200]
        blocks.append(dict(score=int(lines[0][8:]), tname=a[1], tstart=int(a[2]), psize=int(a[3]), tstrand=a[4], tsize=int(a[5]), row_p=a[6].encode(),
                           qname=b[1], qstart=int(b[2]), qsize_row=int(b[3]), qstrand=b[4], qsize=int(b[5]), row_t=b[6].encode()))
    return blocks


def undo(row_p, row_t, eq=None):
    """(the P substring, the T substring, the runs) two rows imply.  A column with two bases is = where they are equal and X where they
    differ -- which is what the rows can say; with eq given (the block's score) the count of = columns is held against it."""
    assert len(row_p) == len(row_t)
    runs = []
    for a, b in zip(row_p, row_t):
        assert not (a == 45 and b == 45)
        op = "I" if a == 45 else "D" if b == 45 else "M" if a == b else "X"
        if runs and runs[-1][1] == op:
            runs[-1] = (runs[-1][0] + 1, op)
        else:
            runs.append((1, op))
    if eq is not None:
        assert eq == sum(n for n, op in runs if op == "M")
    return row_p.replace(b"-", b""), row_t.replace(b"-", b""), runs
