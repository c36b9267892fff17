"""CPU tests of --variants: the model of the variant grammar (tests/variants_model.py) on the example of minimap2's manual and against its
own inverse, the boundary of the new entry points, and the command line without a GPU."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

from tests import cs_model as CS
from tests import left_align_model as M
from tests import variants_model as V
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
R = V.Rec


def test_the_example_of_minimap2s_manual():
    #   CGATCGATAAATAGAGTAG---GAATAGCA
    #   ||||||   ||||||||||   |||| |||
    #   CGATCG---AATAGAGTAGGTCGAATtGCA
    P, T = b"CGATCGATAAATAGAGTAGGAATAGCA", b"CGATCGAATAGAGTAGGTCGAATTGCA"
    runs = M.parse("6=3D10=3I4=1X3=")
    recs, ends = V.variants_of(P, T, runs)
    assert ends == 0
    assert recs == [R(V.DEL, 5, 6, b"GATA", b"G"), R(V.INS, 18, 16, b"G", b"GGTC"), R(V.SNV, 23, 23, b"A", b"T")]
    assert V.apply(P, recs) == T
    assert V.from_cs(CS.cs_of(P, T, runs, CS.SHORT), P) == recs
    assert V.vcf_lines(recs, "chr1", 100, "q", 7, 34, "+") == [
        "chr1\t106\t.\tGATA\tG\t.\t.\tQNAME=q;QSTART=13;QEND=13;QSTRAND=+",
        "chr1\t119\t.\tG\tGGTC\t.\t.\tQNAME=q;QSTART=23;QEND=26;QSTRAND=+",
        "chr1\t124\t.\tA\tT\t.\t.\tQNAME=q;QSTART=30;QEND=31;QSTRAND=+"]
    # on '-' the text is the reverse complement of query [7, 34): its span [u, u + n) is the forward span [34 - u - n, 34 - u)
    assert [l.split("\t")[7] for l in V.vcf_lines(recs, "chr1", 100, "q", 7, 34, "-")] == [
        "QNAME=q;QSTART=28;QEND=28;QSTRAND=-", "QNAME=q;QSTART=15;QEND=18;QSTRAND=-", "QNAME=q;QSTART=10;QEND=11;QSTRAND=-"]


def _random_valid_case(rng):
    """a valid CIGAR without end gaps: M over equal bases, X over different ones; adjacent gaps and gaps behind X runs included"""
    ops, last = [], None
    for k in range(rng.randint(1, 30)):
        op = rng.choice([o for o in "MXID" if o != last])
        ops.append(op)
        last = op
    if ops[0] in "ID":
        ops.insert(0, rng.choice("MX"))
    if ops[-1] in "ID":
        ops.append(rng.choice([o for o in "MX"]))
    runs = []
    for op in ops:  # (inserting the closing run may have put two of one op side by side)
        if runs and runs[-1][1] == op:
            continue
        runs.append((rng.randint(1, 9), op))
    P = bytes(rng.choice(b"ACGT") for _ in range(sum(n for n, o in runs if o != "I")))
    T, p = bytearray(), 0
    for n, op in runs:
        if op == "M":
            T += P[p:p + n]
        elif op == "X":
            T += bytes(rng.choice([c for c in b"ACGT" if c != b]) for b in P[p:p + n])
        elif op == "I":
            T += bytes(rng.choice(b"ACGT") for _ in range(n))
        p += n if op != "I" else 0
    return P, bytes(T), runs


def test_apply_inverts_variants_of_on_random_valid_cigars():
    rng = random.Random(0x7A)
    seen = set()
    for _ in range(400):
        P, T, runs = _random_valid_case(rng)
        recs, ends = V.variants_of(P, T, runs)
        assert ends == 0 and V.apply(P, recs) == T
        # the counts the table gives
        assert len(recs) == sum(n if op == "X" else 1 if op in "ID" else 0 for n, op in runs)
        assert sum(len(r.ref) + len(r.alt) for r in recs) == sum(2 * n if op == "X" else n + 2 if op in "ID" else 0 for n, op in runs)
        assert [r.p for r in recs] == sorted(r.p for r in recs)
        assert V.from_cs(CS.cs_of(P, T, runs, CS.SHORT), P) == recs
        seen |= {a + b for (_, a), (_, b) in zip(runs, runs[1:])}
    assert {"ID", "DI", "XI", "XD"} <= seen


def test_masked_rule():
    recs, _ = V.variants_of(b"ANcg-", b"CTNaT", M.parse("5X"))
    assert [r.kind for r in recs] == [V.SNV, V.SNV | V.MASKED, V.SNV | V.MASKED, V.SNV, V.SNV | V.MASKED]  # N on either side, lower case is a base
    assert [(r.ref, r.alt) for r in recs] == [(b"A", b"C"), (b"N", b"T"), (b"c", b"N"), (b"g", b"a"), (b"-", b"T")]  # bytes as they are
    lines = V.vcf_lines(recs, "t", 0, "q", 0, 5, "+")
    assert [l.split("\t")[1] for l in lines] == ["1", "4"]  # masked SNVs are left out of the file
    # an indel is never masked: its N goes out as it is
    recs, _ = V.variants_of(b"ANNC", b"AC", M.parse("1=2D1="))
    assert recs == [R(V.DEL, 0, 1, b"ANN", b"A")]


def test_end_gaps_are_counted_and_not_called():
    assert V.variants_of(b"ACTCC", b"GGACT", M.parse("2I3=2D")) == ([], 2)
    assert V.variants_of(b"CCACT", b"ACTGG", M.parse("2D3=2I")) == ([], 2)
    assert V.variants_of(b"", b"ACGT", M.parse("4I")) == ([], 1)
    # a D behind a leading I has no pattern base before it: no anchor, an alignment end as well
    assert V.variants_of(b"ACGT", b"TTGT", M.parse("2I2D2=")) == ([], 2)
    # behind a leading D an I has its anchor
    assert V.variants_of(b"ACGT", b"TTGT", M.parse("2D2I2=")) == ([R(V.INS, 1, 0, b"C", b"CTT")], 1)
    # the interior ones between them are called
    recs, ends = V.variants_of(b"AACGTT", b"TACCGT", M.parse("1I1D2=1I2=1D"))
    assert ends == 3 and recs == [R(V.INS, 2, 3, b"C", b"CC")]


def test_entry_points_structures_and_constants():
    L = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfmash_hip.h")).read(), flags=re.S)
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfmash_host.h")).read(), flags=re.S)
    for name in ("wfm_call_variants", "wfm_free_variants"):
        assert re.search(r"\b" + name + r"\s*\(", text) and name in capi.EXPORTS and hasattr(L, name)
    for name in ("wfmh_set_variants", "wfmh_variants_counts"):
        assert re.search(r"\b" + name + r"\s*\(", host) and name in capi.HOST_EXPORTS and hasattr(L, name)
    assert C.sizeof(capi.Variant) == 32
    assert [getattr(capi.Variant, f).offset for f in ("problem", "kind", "p", "t", "ref_len", "alt_len", "off")] == [0, 4, 8, 12, 16, 20, 24]
    assert capi.VARIANT_DTYPE.itemsize == 32 and [capi.VARIANT_DTYPE.fields[f][1] for f in ("problem", "kind", "p", "t", "ref_len", "alt_len", "off")] == [0, 4, 8, 12, 16, 20, 24]
    assert C.sizeof(capi.VarCall) == 32
    assert [getattr(capi.VarCall, f).offset for f in ("flags", "n_runs", "first", "count", "end_gaps")] == [0, 4, 8, 16, 24]
    for name, value in (("WFM_VAR_SNV", capi.WFM_VAR_SNV), ("WFM_VAR_INS", capi.WFM_VAR_INS), ("WFM_VAR_DEL", capi.WFM_VAR_DEL),
                        ("WFM_VAR_MASKED", capi.WFM_VAR_MASKED), ("WFM_VAR_NOT_DONE", capi.WFM_VAR_NOT_DONE), ("WFM_VAR_SPANS", capi.WFM_VAR_SPANS)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)u", text)
        assert m and int(m.group(1)) == value
    m = re.search(r"#define\s+WFM_VAR_SLICE\s+(\d+)\b", text)
    assert m and int(m.group(1)) == capi.WFM_VAR_SLICE
    assert (V.SNV, V.INS, V.DEL, V.MASKED) == (capi.WFM_VAR_SNV, capi.WFM_VAR_INS, capi.WFM_VAR_DEL, capi.WFM_VAR_MASKED)


def test_switch_is_off_by_default_and_its_counts_are_zero(tmp_path):
    assert capi.variants_counts() == (0, 0, 0, 0)
    capi.set_variants(str(tmp_path / "x.vcf"))
    try:
        assert capi.variants_counts() == (0, 0, 0, 0)
    finally:
        capi.set_variants(None)
    assert not (tmp_path / "x.vcf").exists()  # the file is the align phase's to write


def _cli(args, cwd):
    return subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,needles", [
    (["--variants", "out.vcf", "-m", "target.fa"], ["--variants", "cannot be combined with -m"]),
    (["--variants", "out.vcf", "--verify-paf", "x", "target.fa"], ["--variants", "cannot be combined with --verify-paf"]),
], ids=["with_m", "with_verify_paf"])
def test_cli_refusals_before_any_device(tmp_path, args, needles):
    r = _cli(args, tmp_path)
    assert r.returncode == 1
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and all(n in lines[0] for n in needles), r.stderr
    assert "device" not in r.stderr and r.stdout == ""
    assert not (tmp_path / "out.vcf").exists()


def test_cli_help_lists_the_flag(tmp_path):
    r = _cli(["--help"], tmp_path)
    assert r.returncode == 0 and "--variants FILE" in r.stderr + r.stdout
    head = open(os.path.join(ROOT, "wfmash_amd", "host", "main.cpp")).read().split("#include")[0]
    assert "--variants FILE" in head
