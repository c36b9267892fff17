"""CPU tests of --coverage: the model of the depth track (tests/coverage_model.py) on hand cases, the boundary of the new entry points,
the bedGraph writer through its test hook, and the command line without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import coverage_model as V
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")


def test_model_hand_cases():
    assert V.depth_of([(0, V.parse("3=2D3="))], 8).tolist() == [1, 1, 1, 0, 0, 1, 1, 1]
    # two abutting records are one interval, and the word they share is zero
    two = [(2, V.parse("4=")), (6, V.parse("2X1="))]
    assert V.depth_of(two, 12).tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    assert V.entries_of(two, 12) == [(2, 1), (9, -1)]
    assert V.intervals_of(two, 12) == ([(0, 0), (2, 1), (9, 0)], (7, 7, 1))
    # an I changes nothing
    assert V.depth_of([(1, V.parse("2=3I2="))], 6).tolist() == V.depth_of([(1, V.parse("4="))], 6).tolist() == [0, 1, 1, 1, 1, 0]
    assert V.entries_of([(1, V.parse("2=3I2="))], 6) == [(1, 1), (5, -1)]  # (the -1 and the +1 at the I cancel)
    # =/X alternation is one stretch; the -1 of a record that ends the array lands on the word at n_bases
    assert V.entries_of([(0, V.parse("2=1X2="))], 5) == [(0, 1), (5, -1)]
    # overlap adds up
    assert V.intervals_of([(0, V.parse("6=")), (2, V.parse("2=")), (3, V.parse("1X"))], 6) == ([(0, 1), (2, 2), (3, 3), (4, 1)], (6, 9, 3))
    assert V.intervals_of([], 0) == ([(0, 0)], (0, 0, 0)) and V.intervals_of([], 7) == ([(0, 0)], (0, 0, 0))
    assert V.words(V.parse("3=2D1I4X")) == [12, 11, 6, 17]
    assert V.parse("5S3=2H") == [(3, "=")]


def test_model_bedgraph_and_back():
    names, lengths = ["a", "empty", "b", "c"], [6, 0, 4, 3]
    depth = np.array([0, 1, 1, 2, 2, 2, 2, 2, 0, 0, 0, 0, 0])
    text = V.bedgraph(names, lengths, depth)
    assert text == "a\t0\t1\t0\na\t1\t3\t1\na\t3\t6\t2\nb\t0\t2\t2\nb\t2\t4\t0\nc\t0\t3\t0\n"
    back, n = V.parse_bedgraph(text, names, lengths)
    assert back.tolist() == depth.tolist() and n == 6
    for bad in ("a\t0\t6\t0\nb\t0\t4\t0\n",                               # c is missing
                "a\t0\t3\t1\na\t3\t6\t1\nb\t0\t4\t0\nc\t0\t3\t0\n",     # not maximal
                "a\t0\t6\t0\nb\t1\t4\t0\nc\t0\t3\t0\n",                  # a hole
                "b\t0\t4\t0\na\t0\t6\t0\nc\t0\t3\t0\n"):                 # out of order
        with pytest.raises(AssertionError):
            V.parse_bedgraph(bad, names, lengths)


def test_entry_points_structures_and_constants():
    L = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfmash_hip.h")).read(), flags=re.S)
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfmash_host.h")).read(), flags=re.S)
    for name in ("wfm_coverage_create", "wfm_coverage_free", "wfm_coverage_add", "wfm_coverage_export", "wfm_coverage_import",
                 "wfm_coverage_intervals", "wfm_coverage_free_list"):
        assert re.search(r"\b" + name + r"\s*\(", text) and name in capi.EXPORTS and hasattr(L, name)
    for name in ("wfmh_set_coverage", "wfmh_coverage_counts", "wfmh_coverage_paf", "wfmh_test_coverage_bedgraph"):
        assert re.search(r"\b" + name + r"\s*\(", host) and name in capi.HOST_EXPORTS and hasattr(L, name)
    assert C.sizeof(capi.CovProb) == 24 and capi.COV_PROB_DTYPE.itemsize == 24
    assert [getattr(capi.CovProb, f).offset for f in ("base", "runs_off", "n_runs")] == [0, 8, 16]
    assert [capi.COV_PROB_DTYPE.fields[f][1] for f in ("base", "runs_off", "n_runs")] == [0, 8, 16]
    assert C.sizeof(capi.CovEntry) == 16 and capi.COV_ENTRY_DTYPE.itemsize == 16
    assert [getattr(capi.CovEntry, f).offset for f in ("pos", "delta")] == [0, 8] == [capi.COV_ENTRY_DTYPE.fields[f][1] for f in ("pos", "delta")]
    assert C.sizeof(capi.CovInterval) == 16 and capi.COV_INTERVAL_DTYPE.itemsize == 16
    assert [getattr(capi.CovInterval, f).offset for f in ("start", "depth")] == [0, 8] == [capi.COV_INTERVAL_DTYPE.fields[f][1] for f in ("start", "depth")]
    m = re.search(r"#define\s+WFM_COV_SPANS\s+(\d+)u", text)
    assert m and int(m.group(1)) == capi.WFM_COV_SPANS
    for name, value in (("WFM_COV_TILE", capi.WFM_COV_TILE), ("WFM_COV_SCAN_BLOCK", capi.WFM_COV_SCAN_BLOCK)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value
    # a tile is read in 16-byte loads by whole workgroups
    assert capi.WFM_COV_TILE % 1024 == 0 and capi.WFM_COV_SCAN_BLOCK % 256 == 0
    # the align parameters keep their size: the switch is process-wide
    assert C.sizeof(capi.AlignParams) == 88


def _hook(names, lengths, intervals):
    """the writer's text, held against the model's for the same dense depth"""
    text = capi.host_coverage_bedgraph(names, lengths, intervals)
    total = sum(lengths)
    depth = np.zeros(total, dtype=np.int64)
    for k, (a, d) in enumerate(intervals):
        b = intervals[k + 1][0] if k + 1 < len(intervals) else total
        depth[a:b] = d
    assert text == V.bedgraph(names, lengths, depth)
    back, _ = V.parse_bedgraph(text, names, lengths)
    assert back.tolist() == depth.tolist()
    return text


def test_writer_splits_at_sequence_boundaries():
    # one interval of depth 2 over [3, 12) straddles a|b and b|c
    text = _hook(["a", "b", "c"], [5, 4, 6], [(0, 0), (3, 2), (12, 0)])
    assert text == "a\t0\t3\t0\na\t3\t5\t2\nb\t0\t4\t2\nc\t0\t3\t2\nc\t3\t6\t0\n"


def test_writer_untouched_and_empty_sequences():
    text = _hook(["a", "none", "zero", "b"], [5, 7, 0, 3], [(0, 1), (4, 0), (13, 3)])
    assert text == "a\t0\t4\t1\na\t4\t5\t0\nnone\t0\t7\t0\nb\t0\t1\t0\nb\t1\t3\t3\n"
    assert "zero" not in text
    # nothing aligned at all: one line of depth 0 per sequence; an interval that begins exactly at a boundary; a first interval behind 0
    assert _hook(["a", "b"], [2, 3], [(0, 0)]) == "a\t0\t2\t0\nb\t0\t3\t0\n"
    assert _hook(["a", "b"], [2, 3], []) == "a\t0\t2\t0\nb\t0\t3\t0\n"
    assert _hook(["a", "b"], [2, 3], [(0, 4), (2, 1)]) == "a\t0\t2\t4\nb\t0\t3\t1\n"
    assert capi.host_coverage_bedgraph(["a", "b"], [2, 3], [(1, 4)]) == "a\t0\t1\t0\na\t1\t2\t4\nb\t0\t3\t4\n"
    assert capi.host_coverage_bedgraph([], [], [(0, 0)]) == ""


def test_switch_is_off_by_default_and_its_counts_are_zero(tmp_path):
    assert capi.coverage_counts() == (0, 0, 0, 0)
    capi.set_coverage(str(tmp_path / "x.bg"))
    try:
        assert capi.coverage_counts() == (0, 0, 0, 0)
    finally:
        capi.set_coverage(None)
    assert not (tmp_path / "x.bg").exists()  # the file is the align phase's to write


def _cli(args, cwd):
    return subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,needles", [
    (["--coverage", "out.bg", "-m", "target.fa"], ["--coverage", "cannot be combined with -m"]),
    (["--coverage", "out.bg", "--verify-paf", "x", "target.fa"], ["--coverage", "cannot be combined with --verify-paf"]),
    (["--coverage-paf", "in.paf", "target.fa"], ["--coverage-paf", "needs --coverage"]),
    (["--coverage-paf", "in.paf", "--coverage", "out.bg", "--left-align", "target.fa"], ["--coverage-paf", "runs nothing else"]),
    (["--coverage-paf", "in.paf", "--coverage", "out.bg", "-t", "4", "target.fa"], ["--coverage-paf", "runs nothing else"]),
    (["--coverage-paf", "in.paf", "--coverage", "out.bg", "target.fa", "query.fa"], ["--coverage-paf", "runs nothing else"]),
], ids=["with_m", "with_verify_paf", "paf_without_file", "paf_with_left_align", "paf_with_threads", "paf_with_query"])
def test_cli_refusals_before_any_device(tmp_path, args, needles):
    r = _cli(args, tmp_path)
    assert r.returncode == 1
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and all(n in lines[0] for n in needles), r.stderr
    assert "device" not in r.stderr and r.stdout == ""
    assert not (tmp_path / "out.bg").exists()


def test_cli_help_lists_both_flags(tmp_path):
    r = _cli(["--help"], tmp_path)
    assert r.returncode == 0 and "--coverage FILE" in r.stderr + r.stdout and "--coverage-paf FILE" in r.stderr + r.stdout
    head = open(os.path.join(ROOT, "wfmash_amd", "host", "main.cpp")).read().split("#include")[0]
    assert "--coverage FILE" in head and "--coverage-paf IN.paf" in head
