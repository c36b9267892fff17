"""The variants of a problem's runs as wfm_call_variants calls them (include/wfmash_hip.h states the grammar), in plain Python: the
records, their inverse, the VCF lines the align driver writes of them, and the variants a short cs string implies.

Runs are (length, op) with op one of 'M', 'X', 'I', 'D' as in tests/left_align_model.py; P is the pattern (target, REF side), T the text
(query, strand-adjusted), both bytes.  Nothing here is shared with the library.  The records are called from the runs, never from a
comparison."""
import collections
import re

SNV, INS, DEL = 0, 1, 2
MASKED = 256
ACGT = frozenset(b"ACGTacgt")

# kind (with the MASKED bit), p, t, ref, alt: ref and alt are the allele bytes
Rec = collections.namedtuple("Rec", "kind p t ref alt")


def variants_of(P, T, runs):
    """([Rec], end_gaps).  A gap is called unless it is the first or the last run or no pattern base lies before it (p = 0): those are
    counted in end_gaps."""
    out, ends, p, t = [], 0, 0, 0
    for r, (n, op) in enumerate(runs):
        if op == "M":
            p += n
            t += n
        elif op == "X":
            for j in range(n):
                ref, alt = P[p + j:p + j + 1], T[t + j:t + j + 1]
                masked = 0 if ref[0] in ACGT and alt[0] in ACGT else MASKED
                out.append(Rec(SNV | masked, p + j, t + j, ref, alt))
            p += n
            t += n
        else:
            called = 0 < r < len(runs) - 1 and p > 0
            if not called:
                ends += 1
            elif op == "I":
                out.append(Rec(INS, p - 1, t, P[p - 1:p], P[p - 1:p] + T[t:t + n]))
            else:
                out.append(Rec(DEL, p - 1, t, P[p - 1:p + n], P[p - 1:p]))
            if op == "I":
                t += n
            else:
                p += n
    return out, ends


def apply(P, records):
    """the inverse: the records applied to P from the last to the first.  T for every valid CIGAR without end gaps"""
    s = bytearray(P)
    for r in reversed(records):
        kind = r.kind & 255
        if kind == SNV:
            s[r.p:r.p + 1] = r.alt
        elif kind == INS:
            s[r.p + 1:r.p + 1] = r.alt[1:]
        else:
            del s[r.p + 1:r.p + len(r.ref)]
    return bytes(s)


def header(version, contigs):
    """the file's header lines; contigs: [(name, length)] in the target index's order"""
    out = ["##fileformat=VCFv4.2", "##source=wfmash-hip " + version]
    out += ["##contig=<ID=%s,length=%d>" % c for c in contigs]
    out += ['##INFO=<ID=QNAME,Number=1,Type=String,Description="Query sequence name">',
            '##INFO=<ID=QSTART,Number=1,Type=Integer,Description="Start of the query bases in ALT, 0-based, forward strand">',
            '##INFO=<ID=QEND,Number=1,Type=Integer,Description="End of the query bases in ALT, exclusive, forward strand">',
            '##INFO=<ID=QSTRAND,Number=1,Type=String,Description="Strand of the query in the alignment">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    return out


def vcf_lines(records, tname, ts, qname, qs, qe, strand):
    """the lines of one PAF record: ts is the line's target start, [qs, qe) its query interval, strand '+' or '-'.  Masked SNVs are
    left out.  [QSTART, QEND) is the forward-strand query span of the query bases in ALT: one base for an SNV, the inserted bases for an
    INS, an empty span at the junction for a DEL"""
    out = []
    for r in records:
        if r.kind & MASKED:
            continue
        kind = r.kind & 255
        u, n = (r.t, 1) if kind == SNV else (r.t, len(r.alt) - 1) if kind == INS else (r.t, 0)
        a, b = (qs + u, qs + u + n) if strand == "+" else (qe - u - n, qe - u)
        out.append("%s\t%d\t.\t%s\t%s\t.\t.\tQNAME=%s;QSTART=%d;QEND=%d;QSTRAND=%s" % (tname, ts + r.p + 1, r.ref.decode(), r.alt.decode(), qname, a, b, strand))
    return out


_TOKEN = re.compile(rb":(\d+)|\*([^:=*+\-])([^:=*+\-])|\+([^:=*+\-]+)|-([^:=*+\-]+)")


def from_cs(cs, P):
    """the variants a short cs string implies, as [Rec]: the string's bases are lower case, so the alleles take theirs from P where they are
    pattern bases and are upper-cased where they are the query's.  A leading or closing + or - is an alignment end, as in variants_of"""
    tokens, at = [], 0
    while at < len(cs):
        m = _TOKEN.match(cs, at)
        if not m:
            raise ValueError("bad cs at byte %d: %r" % (at, cs[at:at + 20]))
        at = m.end()
        tokens.append(m.groups())
    out, p, t = [], 0, 0
    for k, (n, xa, xb, ins, dele) in enumerate(tokens):
        interior = 0 < k < len(tokens) - 1 and p > 0
        if n is not None:
            p += int(n)
            t += int(n)
        elif xa is not None:
            alt = xb.upper()
            masked = 0 if P[p] in ACGT and alt[0] in ACGT else MASKED
            out.append(Rec(SNV | masked, p, t, P[p:p + 1], alt))
            p += 1
            t += 1
        elif ins is not None:
            if interior:
                out.append(Rec(INS, p - 1, t, P[p - 1:p], P[p - 1:p] + ins.upper()))
            t += len(ins)
        else:
            if interior:
                out.append(Rec(DEL, p - 1, t, P[p - 1:p + len(dele)], P[p - 1:p]))
            p += len(dele)
    return out
