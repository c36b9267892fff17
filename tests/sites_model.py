"""The semantics of --genotypes (include/wfmash_hip.h: wfm_sites_*; include/wfmash_host.h: wfmh_set_genotypes) restated by brute force:
the yardstick of tests/test_sites_cpu.py and tests/test_sites_gpu.py.  Nothing here is shared with the library.

A VARIANT is (pos, kind, group, ref, alt): pos global (over the concatenation of the target's sequences), ref and alt bytes.  Its allele
bytes are folded to upper case.  A SITE is a distinct (pos, ref, alt); lines are biallelic.  Cell (site, g), haploid:
  '1'  some variant of group g is exactly this site;
  '0'  otherwise, if every base of [pos, pos + len(ref)) lies under an = base of at least one record of group g (= only, not X; several
       records of the group may share the span between them; another group's bases never count);
  '.'  otherwise.
One boolean array per group over the concatenation; a '0' is mask[g, pos:pos + len(ref)].all()."""
import numpy as np

from tests import coverage_model as V
from tests import pav_model as PM
from tests import variants_model as VM

SNV, INS, DEL = VM.SNV, VM.INS, VM.DEL
parse, words, offsets = V.parse, V.words, V.offsets
group_key, columns = PM.group_key, PM.columns


def kind_of(ref, alt):
    return SNV if len(ref) == 1 and len(alt) == 1 else INS if len(ref) == 1 else DEL


def eq_mask(problems, n_bases, n_groups):
    """problems = [(base, runs, group)]: per group, the bases under an = run"""
    m = np.zeros((n_groups, n_bases), dtype=bool)
    for base, runs, g in problems:
        p = base
        for n, op in runs:
            if op == "=":
                m[g, p:p + n] = True
            if op != "I":
                p += n
    return m


def eq_segments(problems):
    """how many segments wfm_sites_add_ref appends: one per maximal stretch of = runs"""
    n = 0
    for _, runs, _ in problems:
        prev = "D"
        for _, op in runs:
            n += op == "=" and prev != "="
            prev = op
    return n


def table(variants, problems, n_bases, n_groups):
    """(sites, rows): sites = [(pos, ref, alt)] folded, sorted by (pos, ref, alt); rows[s] = a string of n_groups cells.  Also returns,
    third, the number of distinct carrier groups per site"""
    carriers = {}
    for pos, kind, g, ref, alt in variants:
        assert kind == kind_of(ref, alt)
        carriers.setdefault((pos, ref.upper(), alt.upper()), set()).add(g)
    mask = eq_mask(problems, n_bases, n_groups)
    sites = sorted(carriers)
    rows = []
    for pos, ref, alt in sites:
        has = carriers[(pos, ref, alt)]
        rows.append("".join("1" if g in has else "0" if mask[g, pos:pos + len(ref)].all() else "." for g in range(n_groups)))
    return sites, rows, [len(carriers[s]) for s in sites]


def header(version, contigs, cols):
    """--variants' header lines, AC and AN, GT, and the column line with one column per group"""
    h = VM.header(version, contigs)
    return h[:-1] + ['##INFO=<ID=AC,Number=A,Type=Integer,Description="Groups that carry ALT">',
                     '##INFO=<ID=AN,Number=1,Type=Integer,Description="Groups with a called allele, REF or ALT">',
                     '##FORMAT=<ID=GT,Number=1,Type=String,Description="Haploid genotype of the group: 1 carries ALT, 0 has REF under = bases, . neither">',
                     "\t".join([h[-1], "FORMAT"] + list(cols))]


def line(tname, pos1, ref, alt, cells):
    return "\t".join([tname, str(pos1), ".", ref.decode(), alt.decode(), ".", ".", "AC=%d;AN=%d" % (cells.count("1"), cells.count("1") + cells.count("0")), "GT"]
                     + list(cells))


def body(tnames, tlengths, sites, rows):
    """the lines, sorted by (sequence in index order, POS, REF bytes, ALT bytes): global order of (pos, ref, alt) is just that"""
    off = offsets(tlengths)
    out = []
    for (pos, ref, alt), cells in sorted(zip(sites, rows)):
        c = int(np.searchsorted(off, pos, side="right")) - 1
        while tlengths[c] == 0:  # (an empty sequence shares its offset with the next one)
            c += 1
        assert pos + len(ref) <= off[c + 1], "a site straddles two sequences"
        out.append(line(tnames[c], pos - int(off[c]) + 1, ref, alt, cells))
    return out


def inputs_of_paf(lines, bases_of, split, tnames, tlengths, cols, delim="#"):
    """aligned PAF lines as (variants, = problems): bases_of(fields) -> (P, T), the target's and the strand-adjusted query's bases of the
    line; split(line) -> (fields, cigar).  Masked SNVs are left out, as in --variants.  Returns the number left out third"""
    off = offsets(tlengths)
    variants, problems, masked = [], [], 0
    for text in lines:
        f, cg = split(text)
        runs = parse(cg)
        base = int(off[tnames.index(f[5])]) + int(f[7])
        g = cols.index(group_key(f[0], delim))
        P, T = bases_of(f)
        recs, ends = VM.variants_of(P, T, [(n, "M" if op == "=" else op) for n, op in runs])
        assert ends == 0
        for r in recs:
            if r.kind & VM.MASKED:
                masked += 1
                continue
            variants.append((base + r.p, r.kind, g, r.ref, r.alt))
        problems.append((base, runs, g))
    return variants, problems, masked


def file_of(version, tnames, tlengths, cols, variants, problems):
    """the --genotypes file as a list of lines"""
    sites, rows, _ = table(variants, problems, int(offsets(tlengths)[-1]), len(cols))
    return header(version, list(zip(tnames, tlengths)), cols) + body(tnames, tlengths, sites, rows)
