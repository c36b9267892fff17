"""CPU tests of --genotypes: the brute-force model (tests/sites_model.py) against hand-computed cases, the text side of the driver (header,
AC / AN, the order of the lines) through its test hook against the model's lines, the command line's refusals and the new exports, all
without a GPU."""
import ctypes
import os
import subprocess

import pytest

from tests import sites_model as M
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
P = M.parse
SNV, INS, DEL = M.SNV, M.INS, M.DEL


def test_model_cells_by_hand():
    variants = [(10, SNV, 0, b"A", b"G"), (10, SNV, 1, b"a", b"g"), (10, SNV, 3, b"A", b"T")]
    problems = [(5, P("5=1X5="), 0), (8, P("2=1X9="), 1), (0, P("30="), 2), (5, P("5=1X5="), 3), (2, P("6=6D6="), 4), (0, P("10="), 5), (11, P("4="), 5)]
    sites, rows, carriers = M.table(variants, problems, 40, 7)
    assert sites == [(10, b"A", b"G"), (10, b"A", b"T")]  # a against A is one site; (pos, REF, ALT) order
    # carried, carried (soft-masked), = there, an X that spells another ALT, under a deletion, a hole of one base, no record at all
    assert rows == ["110....", "..01..."] and carriers == [2, 1]


def test_model_spans_and_groups():
    dele = [(10, DEL, 0, b"ACGTAC", b"A")]
    own = [(4, P("7=5D8="), 0)]
    assert M.table(dele, own + [(4, P("9="), 1), (13, P("7="), 1)], 40, 2)[1] == ["10"]   # two abutting records of one group
    assert M.table(dele, own + [(4, P("9="), 1), (14, P("6="), 1)], 40, 2)[1] == ["1."]   # one base short
    assert M.table(dele, own + [(4, P("9="), 1), (13, P("7="), 2)], 40, 3)[1] == ["1.."]  # the other half is another group's
    assert M.table(dele, own + [(4, P("7=1X6="), 1)], 40, 2)[1] == ["1."]                 # = and X together cover it: not a 0
    # 1 wins over 0 where overlapping records of one group disagree
    assert M.table([(10, SNV, 0, b"A", b"G")], [(5, P("5=1X5="), 0), (0, P("30="), 0)], 40, 1)[1] == ["1"]
    # two insertions at one anchor: 0 on the other's line, 1 on its own; an I takes no target base
    sites, rows, _ = M.table([(10, INS, 0, b"A", b"ACC"), (10, INS, 1, b"A", b"AT")], [(5, P("6=2I5="), 0), (5, P("6=1I5="), 1)], 40, 2)
    assert list(zip(sites, rows)) == [((10, b"A", b"ACC"), "10"), ((10, b"A", b"AT"), "01")]
    assert M.eq_segments([(0, P("3=1X2=2I4=1D1="), 0)]) == 4 and M.eq_mask([(2, P("3=1X2=2I4=1D1="), 0)], 16, 1)[0].tolist() == \
        [False, False, True, True, True, False, True, True, True, True, True, True, False, True, False, False]


def test_model_inputs_of_paf():
    tnames, tlens = ["t#1#a", "t#1#b"], [30, 20]
    seqs = {"t#1#b": b"ACGTACGTACGTACGTACGT"}
    #            target  ACGTAC GT ACGTAC  (from 2: GTACGT AC GTACGT); the query has an X at p = 1, deletes 2 bases and inserts one
    line = "q#2#x\t40\t0\t13\t+\tt#1#b\t20\t2\t16\t11\t15\t60\tcg:Z:1=1X4=2D3=1I3="
    P_, T_ = seqs["t#1#b"][2:16], b"GAACGT" + b"GTA" + b"N" + b"CGT"
    cols = M.columns(["q#1#y", "q#2#x"])
    split = lambda l: (l.split("\t"), l.split("cg:Z:")[1])
    variants, problems, masked = M.inputs_of_paf([line], lambda f: (P_, T_), split, tnames, tlens, cols)
    assert problems == [(32, P("1=1X4=2D3=1I3="), 1)] and masked == 0
    assert variants == [(33, SNV, 1, b"T", b"A"), (37, DEL, 1, b"TAC", b"T"), (42, INS, 1, b"A", b"AN")]
    lines = M.file_of("v", tnames, tlens, cols, variants, problems)
    assert lines[-3:] == ["t#1#b\t4\t.\tT\tA\t.\t.\tAC=1;AN=1\tGT\t.\t1", "t#1#b\t8\t.\tTAC\tT\t.\t.\tAC=1;AN=1\tGT\t.\t1",
                          "t#1#b\t13\t.\tA\tAN\t.\t.\tAC=1;AN=1\tGT\t.\t1"]


def test_text_side_against_the_model():
    """the header, AC / AN, the tie order at one POS whatever order the ties come in, a group without a record as a column of '.', a
    sequence of length 0 before the one a site lies in"""
    tnames, tlens = ["t#1#a", "t#1#empty", "t#1#b"], [100, 0, 50]
    cols = M.columns(["q#3#z", "q#1#y", "q#2#x", "lonely#1"])
    assert cols == ["lonely", "q#1", "q#2", "q#3"]
    g = cols.index
    variants = [(10, SNV, g("q#1"), b"A", b"T"), (10, SNV, g("q#2"), b"A", b"G"), (10, INS, g("q#3"), b"A", b"AG"), (10, DEL, g("q#3"), b"AC", b"A"),
                (10, INS, g("q#1"), b"A", b"AGG"), (0, SNV, g("q#1"), b"C", b"A"), (100, SNV, g("q#2"), b"G", b"C"), (149, SNV, g("q#2"), b"T", b"C"),
                (10, SNV, g("q#3"), b"a", b"t")]
    problems = [(0, P("100="), g("q#1")), (5, P("5=1X20="), g("q#2")), (100, P("1X48=1X"), g("q#2")), (100, P("50="), g("q#3"))]
    sites, rows, _ = M.table(variants, problems, 150, len(cols))
    want = M.header("1.2.3", list(zip(tnames, tlens)), cols) + M.body(tnames, tlens, sites, rows)
    assert [l.split("\t")[:5] for l in want if l.startswith("t#1#a\t11\t")] == [
        ["t#1#a", "11", ".", "A", "AG"], ["t#1#a", "11", ".", "A", "AGG"], ["t#1#a", "11", ".", "A", "G"], ["t#1#a", "11", ".", "A", "T"],
        ["t#1#a", "11", ".", "AC", "A"]]  # (REF bytes, then ALT bytes: "A" < "AC", "AG" < "AGG" < "G" < "T")
    assert "t#1#a\t11\t.\tA\tT\t.\t.\tAC=2;AN=2\tGT\t.\t1\t.\t1" in want  # q#2's X spells G there; lonely has no record
    assert "t#1#b\t1\t.\tG\tC\t.\t.\tAC=1;AN=2\tGT\t.\t.\t1\t0" in want and "t#1#b\t50\t.\tT\tC\t.\t.\tAC=1;AN=2\tGT\t.\t.\t1\t0" in want
    assert all(l.split("\t")[9] == "." for l in want if not l.startswith("#"))
    assert want[len(tnames) + 2 + 4:len(tnames) + 2 + 8] == [
        '##INFO=<ID=AC,Number=A,Type=Integer,Description="Groups that carry ALT">',
        '##INFO=<ID=AN,Number=1,Type=Integer,Description="Groups with a called allele, REF or ALT">',
        '##FORMAT=<ID=GT,Number=1,Type=String,Description="Haploid genotype of the group: 1 carries ALT, 0 has REF under = bases, . neither">',
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tlonely\tq#1\tq#2\tq#3"]
    for order in (lambda s: s, lambda s: -len(s[1]) - len(s[2]), lambda s: s[2][::-1]):
        # ascending pos, the ties in three different orders: the device's is a function of its hash
        pairs = sorted(zip(sites, rows), key=lambda sr: (sr[0][0], order(sr[0])))
        got = capi.host_genotype_text("1.2.3", tnames, tlens, cols, [s for s, _ in pairs], [r for _, r in pairs])
        assert got.endswith("\n") and got.splitlines() == want
    # no site at all: the header alone; no group at all: lines without cells
    assert capi.host_genotype_text("v", tnames, tlens, cols, [], []).splitlines() == M.header("v", list(zip(tnames, tlens)), cols)
    assert capi.host_genotype_text("v", ["t"], [9], [], [(3, b"A", b"C")], [""]).splitlines()[-1] == "t\t4\t.\tA\tC\t.\t.\tAC=0;AN=0\tGT"


@pytest.mark.parametrize("args, message", [
    (["--genotypes", "x.vcf", "-m"], "--genotypes reads alignments: it cannot be combined with -m"),
    (["--genotypes", "x.vcf", "--verify-paf", "x.paf"], "--genotypes belongs to the align phase: it cannot be combined with --verify-paf"),
    (["--genotypes"], "need a target FASTA"),  # (its value is missing: "t.fa" is taken for it, and no target is left)
    (["--pav", "x.bed", "--pav-out", "x.tsv", "--pav-paf", "x.paf", "--genotypes", "x.vcf"], "--pav-paf runs nothing else"),
    (["--chain", "x.chain", "--chain-paf", "x.paf", "--genotypes", "x.vcf"], "--chain-paf runs nothing else"),
])
def test_cli_refusals(args, message):
    r = subprocess.run([CLI] + args + ["t.fa"], capture_output=True, text=True)
    assert r.returncode == 1 and message in r.stderr + r.stdout, (r.returncode, r.stderr)


def test_cli_usage_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--genotypes FILE" in r.stdout + r.stderr


def test_the_exports_are_in_the_library():
    lib = ctypes.CDLL(capi.LIB_PATH)
    names = ["wfm_sites_create", "wfm_sites_free", "wfm_sites_add_variants", "wfm_sites_add_ref", "wfm_sites_table", "wfm_sites_export", "wfm_sites_import",
             "wfm_sites_counts", "wfm_sites_free_list", "wfmh_set_genotypes", "wfmh_genotypes_counts", "wfmh_test_genotype_text"]
    assert [n for n in names if not hasattr(lib, n)] == []
    assert set(names[:9]) <= set(capi.EXPORTS)
    assert hasattr(capi, "Sites") and hasattr(capi.Handle, "sites")
    # the switch and its counts need no device
    capi.set_genotypes("/nonexistent/x.vcf")
    capi.set_genotypes(None)
    assert capi.genotypes_counts() == (0, 0, 0, 0)
