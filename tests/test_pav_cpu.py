"""CPU tests of --pav: the brute-force model (tests/pav_model.py) against hand-computed cases, the text side of the driver (group keys,
columns, windows, header and rows) through its test hook against the model byte for byte, and the command line's refusals, all without
a GPU."""
import os
import subprocess

import pytest

from tests import pav_model as M
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
P = M.parse


@pytest.mark.parametrize("name,key", [
    ("chr1", "chr1"),             # no delimiter: the sequence is its own group
    ("sample#", "sample"),        # the delimiter last
    ("a#1#chr", "a#1"),           # two delimiters: the part before the LAST one
    ("#x", ""),
    ("", ""),
])
def test_group_key(name, key):
    assert M.group_key(name) == key
    text = capi.host_pav_text([name], [], [], 1)
    assert text.splitlines()[0] == "#key\t%s\t%s\t0" % (name, key)


def test_columns_are_sorted_bytewise_and_keep_an_empty_group():
    names = ["b#1#x", "a#2#y", "b#1#z", "Z#1#c", "solo", "a#10#y", "a#2#q", "\xc3\xa9#1#c"]
    cols = M.columns(names)
    assert cols == ["Z#1", "a#10", "a#2", "b#1", "solo", "\xc3\xa9#1"]  # ('Z' < 'a'; "a#10" < "a#2"; the high bytes last)
    lines = capi.host_pav_text(names, ["t"], [0], 5).splitlines()
    assert lines[:len(names)] == ["#key\t%s\t%s\t%d" % (n, M.group_key(n), cols.index(M.group_key(n))) for n in names]
    assert lines[len(names)] + "\n" == M.header(cols)
    # a group whose sequences have no record is a column all the same: the model's table has it, all zeros
    problems = [(0, P("5="), cols.index("a#2"))]
    table = M.file_of(["t"], [10], cols, [(0, 0, 10, "g")], problems)
    assert table == M.header(cols) + "t\t0\t10\tg\t10\t0\t0\t5\t0\t0\t0\n"


def test_windows_header_and_rows_byte_for_byte():
    tnames, tlens = ["t#1#a", "t#1#empty", "t#1#b", "t#1#c"], [2500, 0, 1000, 1]
    qnames = ["q#1#a", "q#2#a", "q#1#b"]
    assert M.windows(tnames, tlens, 1000) == [(0, 0, 1000), (0, 1000, 2000), (0, 2000, 2500), (2, 0, 1000), (3, 0, 1)]
    cols = M.columns(qnames)
    want = "".join("#key\t%s\t%s\t%d\n" % (n, M.group_key(n), cols.index(M.group_key(n))) for n in qnames) + M.header(cols)
    for j, (c, a, b) in enumerate(M.windows(tnames, tlens, 1000)):
        want += M.row(tnames[c], a, b, ".", [j + g for g in range(len(cols))])
    got = capi.host_pav_text(qnames, tnames, tlens, 1000)
    assert got == want
    assert "#tname\ttstart\ttend\tname\tlen\tq#1\tq#2\n" in got and "t#1#a\t2000\t2500\t.\t500\t2\t3\n" in got and "t#1#empty" not in got
    # a window as long as the longest sequence, and a longer one
    for size in (2500, 1 << 40):
        rows = capi.host_pav_text(qnames, tnames, tlens, size).splitlines()[len(qnames) + 1:]
        assert [r.split("\t")[:3] for r in rows] == [["t#1#a", "0", "2500"], ["t#1#b", "0", "1000"], ["t#1#c", "0", "1"]]


def test_model_by_hand():
    # two records of one group over the same bases count once; a D base is absent; an I run advances nothing; groups never merge
    problems = [(2, P("4=2D3=2I1X"), 0), (4, P("6="), 0), (4, P("6="), 1)]
    mask = M.mask_of(problems, 20, 3)
    assert M.union_of(mask) == [(2, 10, 0), (4, 6, 1)]
    assert M.matrix_of(mask, [(0, 20), (0, 3), (5, 7), (11, 20), (6, 6)]) == [[10, 6, 0], [1, 0, 0], [2, 2, 0], [1, 0, 0], [0, 0, 0]]
    assert M.segments_of(problems) == 5  # (4= | 3= | 1X, the I between the last two included: stretches, not bases)
    # abutting records merge; an interval wholly inside a deletion gives 0
    mask = M.mask_of([(0, P("5="), 0), (5, P("5=10D5="), 0)], 30, 1)
    assert M.union_of(mask) == [(0, 10, 0), (20, 5, 0)]
    assert M.matrix_of(mask, [(10, 20), (9, 21), (0, 30)]) == [[0], [2], [15]]


def test_model_problems_of_paf():
    names, lengths = ["t#1#a", "t#1#b"], [100, 50]
    lines = ["q#2#x\t40\t0\t12\t+\tt#1#b\t50\t10\t24\t12\t14\t60\tcg:Z:6=2D6=",
             "q#1#y\t40\t0\t5\t-\tt#1#a\t100\t95\t100\t5\t5\t60\tcg:Z:5="]
    cols = M.columns(["q#1#y", "q#2#x", "q#3#z"])
    assert M.problems_of_paf(lines, names, lengths, cols) == [(110, P("6=2D6="), 1), (95, P("5="), 0)]
    table = M.file_of(names, lengths, cols, [(0, 90, 100, "end"), (1, 0, 50, ".")], M.problems_of_paf(lines, names, lengths, cols))
    assert table == "#tname\ttstart\ttend\tname\tlen\tq#1\tq#2\tq#3\nt#1#a\t90\t100\tend\t10\t5\t0\t0\nt#1#b\t0\t50\t.\t50\t0\t12\t0\n"


@pytest.mark.parametrize("args, message", [
    (["--pav", "x.bed"], "--pav needs --pav-out FILE"),
    (["--pav-window", "1000"], "--pav-window needs --pav-out FILE"),
    (["--pav-out", "x.tsv"], "--pav-out needs --pav IN.bed or --pav-window N"),
    (["--pav", "x.bed", "--pav-window", "1000", "--pav-out", "x.tsv"], "--pav IN.bed and --pav-window N exclude each other"),
    (["--pav-window", "0", "--pav-out", "x.tsv"], "--pav-window takes a positive number of bases"),
    (["--pav-window", "1k", "--pav-out", "x.tsv"], "--pav-window takes a positive number of bases"),
    (["--pav-paf", "x.paf"], "--pav-paf needs --pav IN.bed or --pav-window N, and --pav-out FILE"),
    (["--pav", "x.bed", "--pav-out", "x.tsv", "-m"], "--pav reads alignments: it cannot be combined with -m"),
    (["--pav-window", "500", "--pav-out", "x.tsv", "--verify-paf", "x.paf"], "--pav belongs to the align phase: it cannot be combined with --verify-paf"),
    (["--pav", "x.bed", "--pav-out", "x.tsv", "--pav-paf", "x.paf", "--left-align"], "--pav-paf runs nothing else"),
    (["--pav", "x.bed", "--pav-out", "x.tsv", "--pav-paf", "x.paf", "q.fa", "third.fa"], "--pav-paf runs nothing else"),
])
def test_cli_refusals(args, message):
    r = subprocess.run([CLI] + args + ["t.fa"], capture_output=True, text=True)
    assert r.returncode == 1 and message in r.stderr, (r.returncode, r.stderr)


def test_cli_usage_names_the_options():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and "--pav BED | --pav-window N, --pav-out FILE" in text and "--pav-paf FILE" in text
