"""CPU tests of --lift: the brute-force model of a lift (tests/lift_model.py) against hand-written expectations for each rule, the text
side (BED parser, strand arithmetic, line writer) through its test hook against the model byte for byte, and the command line's refusals,
all without a GPU."""
import os
import random
import subprocess

import pytest

from tests import lift_model as M
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")


def one(cigar, start, end, base=0, n_bases=10 ** 6):
    lifts, per = M.lift_problems([(base, M.parse(cigar))], [(start, end)], n_bases)
    assert per[0][0] == 0 and per[0][3] == len(lifts)
    return [lf[2:] for lf in lifts]


def test_model_rules():
    # the whole span, and strictly inside one = run
    assert one("10=", 0, 10) == [(0, 10, 0, 10, 10, 0)]
    assert one("10=", 3, 7) == [(3, 7, 3, 7, 4, 0)]
    # X columns count in x
    assert one("3=2X4=", 2, 6) == [(2, 6, 2, 6, 2, 2)]
    # an endpoint in a D run snaps inward: 4= 3D 4=, pattern 0..10, text 0..7
    assert one("4=3D4=", 5, 9) == [(7, 9, 4, 6, 2, 0)]
    assert one("4=3D4=", 2, 6) == [(2, 4, 2, 4, 2, 0)]
    # wholly inside a D run: present in the target, absent from the query, at the text index reached
    assert one("4=3D4=", 4, 7) == [(4, 4, 4, 4, 0, 0)]
    assert one("4=3D4=", 5, 6) == [(5, 5, 4, 4, 0, 0)]
    # a chain of gaps: 3D then 2I; and 2I then 3D (the text index at the D already holds the I)
    assert one("4=3D2I4=", 4, 7) == [(4, 4, 4, 4, 0, 0)]
    assert one("4=2I3D4=", 4, 7) == [(4, 4, 6, 6, 0, 0)]
    # an I strictly inside is inside [t0, t1); directly before p0 or behind p1 - 1 it is outside
    assert one("4=2I4=", 2, 6) == [(2, 6, 2, 8, 4, 0)]
    assert one("4=2I4=", 4, 8) == [(4, 8, 6, 10, 4, 0)]
    assert one("4=2I4=", 0, 4) == [(0, 4, 0, 4, 4, 0)]
    # gaps at the ends of the run list
    assert one("2I5=", 0, 5) == [(0, 5, 2, 7, 5, 0)]
    assert one("5=2I", 0, 5) == [(0, 5, 0, 5, 5, 0)]
    assert one("2D5=", 0, 7) == [(2, 7, 0, 5, 5, 0)]
    assert one("5=2D", 0, 7) == [(0, 5, 0, 5, 5, 0)]
    assert one("5=2D", 5, 7) == [(5, 5, 5, 5, 0, 0)]
    # clipping, with a base: the span is [100, 110)
    assert one("10=", 90, 105, base=100) == [(0, 5, 0, 5, 5, 0)]
    assert one("10=", 105, 200, base=100) == [(5, 10, 5, 10, 5, 0)]
    assert one("10=", 0, 1000, base=100) == [(0, 10, 0, 10, 10, 0)]
    # touching is not overlapping
    assert one("10=", 90, 100, base=100) == [] and one("10=", 110, 120, base=100) == []
    assert one("10=", 99, 101, base=100) == [(0, 1, 0, 1, 1, 0)]


def test_model_problems_and_flags():
    iv = [(0, 100), (5, 8), (5, 8), (20, 30)]
    lifts, per = M.lift_problems([(2, M.parse("10=")), (0, M.parse("3=0D2=")), (95, M.parse("10=")), (25, [])], iv, 100)
    assert per == [(0, 1, 0, 3), (M.LIFT_SPANS, 3, 3, 0), (M.LIFT_SPANS, 1, 3, 0), (M.LIFT_SPANS, 0, 3, 0)]
    assert lifts == [(0, 0, 0, 10, 0, 10, 10, 0), (0, 1, 3, 6, 3, 6, 3, 0), (0, 2, 3, 6, 3, 6, 3, 0)]
    assert M.words(M.parse("3=2D1I4X")) == [12, 11, 6, 17]


NAMES, LENGTHS = ["t#1#chr1", "t#1#chr2", "track1"], [1000, 400, 50]

BED = "\n".join([
    "# a comment",
    "track name=genes",
    "browser position chr1:1-100",
    "",
    " \t ",
    "t#1#chr2\t10\t50\tgeneB\t0\t+",
    "t#1#chr1\t100\t200\tgeneA",
    "t#1#chr1\t100\t200\tgeneA.dup",          # a duplicate interval: input order breaks the tie
    "t#1#chr1\t0\t1000",                       # no name column
    "t#1#chr1\t150\t160\t",                    # an empty name column
    "t#1#chr9\t1\t2\tunknown",
    "t#1#chr1\t7\t7\tempty",
    "t#1#chr1\t9\t7\tbackwards",
    "t#1#chr2\t390\t401\tbeyond",
    "t#1#chr2\t390\t400\tto_the_end\r",
    "t#1#chr1\t1\t2x\tjunk",
    "t#1#chr1\t-1\t2\tjunk",
    "t#1#chr1\t1",
    "t#1#chr1 5 9 spaces",
    "track1\t0\t50\ta sequence named like a track line",
    "t#1#chr1\t5\t1234567890123456789\ttoo_long",
]) + "\n"


def spec_of(recs, lifts):
    return "".join("R\t%s\t%d\t%d\t%s\t%s\t%d\n" % r for r in recs) + "".join("L\t" + "\t".join(str(v) for v in lf) + "\n" for lf in lifts)


def test_bed_parser_hook_matches_the_model():
    iv, skipped = M.parse_bed(BED, NAMES, LENGTHS)
    assert skipped == 14
    assert [(v["name"], v["gstart"], v["gend"], v["order"]) for v in iv] == [
        (".", 0, 1000, 3), ("geneA", 100, 200, 1), ("geneA.dup", 100, 200, 2), (".", 150, 160, 4), ("geneB", 1010, 1050, 0),
        ("to_the_end", 1390, 1400, 5), ("a sequence named like a track line", 1400, 1450, 6)]
    assert capi.host_lift_lines(NAMES, LENGTHS, BED, "") == M.bed_dump(iv, skipped)
    # no trailing newline, and nothing at all
    for text in (BED[:-1], "", "\n", "t#1#chr1\t1\t2"):
        assert capi.host_lift_lines(NAMES, LENGTHS, text, "") == M.bed_dump(*M.parse_bed(text, NAMES, LENGTHS))
    assert M.parse_bed("\n", NAMES, LENGTHS) == ([], 1) and M.parse_bed("", NAMES, LENGTHS) == ([], 0)


def test_lines_hook_matches_the_model_on_both_strands():
    iv, skipped = M.parse_bed(BED, NAMES, LENGTHS)
    recs = [("q#1#a", 1000, 1300, "+", "t#1#chr1", 90), ("q#1#b", 500, 800, "-", "t#1#chr1", 90), ("q#2#c", 0, 40, "-", "t#1#chr2", 1010 - 1000)]
    lifts = [(0, 1, 10, 110, 12, 115, 95, 3), (1, 1, 10, 110, 12, 115, 95, 3), (0, 3, 60, 60, 70, 70, 0, 0), (1, 3, 60, 60, 70, 70, 0, 0),
             (2, 4, 0, 40, 0, 40, 38, 2), (1, 0, 0, 300, 0, 300, 300, 0)]
    want = M.bed_dump(iv, skipped) + "".join(M.lift_line(recs[lf[0]], iv[lf[1]], NAMES, lf[2:]) for lf in lifts)
    assert capi.host_lift_lines(NAMES, LENGTHS, BED, spec_of(recs, lifts)) == want
    # by hand: + adds to the window's start, - counts back from its end; ins and del are derived
    lines = want.splitlines()[1 + len(iv):]
    assert lines[0] == "q#1#a\t1012\t1115\tgeneA\t+\tt#1#chr1\t100\t200\t100\t200\t95\t3\t5\t2"
    assert lines[1] == "q#1#b\t685\t788\tgeneA\t-\tt#1#chr1\t100\t200\t100\t200\t95\t3\t5\t2"
    assert lines[2] == "q#1#a\t1070\t1070\t.\t+\tt#1#chr1\t150\t150\t150\t160\t0\t0\t0\t0"
    assert lines[3] == "q#1#b\t730\t730\t.\t-\tt#1#chr1\t150\t150\t150\t160\t0\t0\t0\t0"
    assert lines[4] == "q#2#c\t0\t40\tgeneB\t-\tt#1#chr2\t10\t50\t10\t50\t38\t2\t0\t0"


def test_lines_hook_fuzz():
    rng = random.Random(0x11F7)
    iv, skipped = M.parse_bed(BED, NAMES, LENGTHS)
    recs, lifts = [], []
    for k in range(40):
        qs = rng.randrange(0, 10 ** 9)
        recs.append(("q%d" % k, qs, qs + 5000, rng.choice("+-"), rng.choice(NAMES), rng.randrange(0, 10 ** 10)))
        for _ in range(5):
            p0, t0 = rng.randrange(0, 2000), rng.randrange(0, 2000)
            eq, x = rng.randrange(0, 500), rng.randrange(0, 50)
            lifts.append((k, rng.randrange(len(iv)), p0, p0 + eq + x + rng.randrange(0, 99), t0, t0 + eq + x + rng.randrange(0, 99), eq, x))
    want = M.bed_dump(iv, skipped) + "".join(M.lift_line(recs[lf[0]], iv[lf[1]], NAMES, lf[2:]) for lf in lifts)
    assert capi.host_lift_lines(NAMES, LENGTHS, BED, spec_of(recs, lifts)) == want


def test_hook_refuses_a_spec_it_cannot_read():
    for spec in ("L\t0\t0\t1\t2\t3\t4\t5\t6\n", "R\tq\t1\t2\t+\tt\n", "X\n", "R\tq\t1\t2\t+\tt\t0\nL\t0\t99\t1\t2\t3\t4\t5\t6\n"):
        with pytest.raises(capi.WfmError):
            capi.host_lift_lines(NAMES, LENGTHS, BED, spec)


def test_model_lift_paf():
    paf = ["q\t500\t98\t111\t-\tt#1#chr1\t1000\t95\t109\t9\t15\t60\tcg:Z:4=3D2I3=1X3=\n"]
    text, counts = M.lift_paf(paf, "t#1#chr1\t90\t100\tA\nt#1#chr1\t99\t102\tB\nt#1#chr1\t0\t1000\n#x\n", NAMES, LENGTHS)
    # sorted: the whole sequence, A, B; the span is [95, 109), the text 13 bases
    assert text == ("q\t98\t111\t.\t-\tt#1#chr1\t95\t109\t0\t1000\t10\t1\t2\t3\n"
                    "q\t107\t111\tA\t-\tt#1#chr1\t95\t99\t90\t100\t4\t0\t0\t0\n"
                    "q\t107\t107\tB\t-\tt#1#chr1\t99\t99\t99\t102\t0\t0\t0\t0\n")
    assert counts == (1, 3, 1, 1)


@pytest.mark.parametrize("args, message", [
    (["--lift", "x.bed"], "--lift needs --lift-out FILE"),
    (["--lift-out", "x.tsv"], "--lift-out needs --lift IN.bed"),
    (["--lift-paf", "x.paf"], "--lift-paf needs --lift IN.bed and --lift-out FILE"),
    (["--lift", "x.bed", "--lift-out", "x.tsv", "-m"], "--lift lifts through alignments: it cannot be combined with -m"),
    (["--lift", "x.bed", "--lift-out", "x.tsv", "--verify-paf", "x.paf"], "--lift belongs to the align phase: it cannot be combined with --verify-paf"),
    (["--lift", "x.bed", "--lift-out", "x.tsv", "--lift-paf", "x.paf", "-t", "2"], "--lift-paf runs nothing else"),
    (["--lift", "x.bed", "--lift-out", "x.tsv", "--lift-paf", "x.paf", "q.fa"], "--lift-paf runs nothing else"),
])
def test_cli_refusals(args, message):
    r = subprocess.run([CLI] + args + ["t.fa"], capture_output=True, text=True)
    assert r.returncode == 1 and message in r.stderr, (r.returncode, r.stderr)


def test_cli_usage_names_the_options():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and "--lift BED --lift-out FILE" in text and "--lift-paf FILE" in text
