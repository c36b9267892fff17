"""CPU tests of --left-align: the rule's model (tests/left_align_model.py) held against itself on seeded cases built by construction,
the hand cases with their expected CIGARs written out, the boundary of the new entry points, and the command line without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import left_align_cases as LC
from tests import left_align_model as M
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
PENS = [(5, 8, 2, 24, 1), (3, 4, 2, 24, 1)]


@pytest.fixture(scope="module")
def cases():
    return M.seeded_cases(300)


def test_planted_cases_are_valid_and_hold_movable_gaps(cases):
    assert len(cases) == 300
    for P, T, runs in cases:
        assert M.check(P, T, runs) is None
    assert sum(len(M.movable(P, T, runs)) for P, T, runs in cases) > 300  # the generator plants what the rule is about


def test_model_against_itself(cases):
    gaps = moved = 0
    for P, T, runs in cases:
        out, shifts = M.left_align(P, T, runs)
        assert M.check(P, T, out) is None, (M.spell(runs), M.spell(out))
        assert M.counts(out) == M.counts(runs)
        for pen in PENS:
            assert M.price(out, pen) == M.price(runs, pen)
        again, shifts2 = M.left_align(P, T, out)
        assert again == out and not any(shifts2)
        assert M.movable(P, T, out) == [], (M.spell(runs), M.spell(out))
        assert out[0][1] == runs[0][1] and out[-1][1] == runs[-1][1]
        if runs[0][1] in "ID":
            assert out[0] == runs[0]
        if runs[-1][1] in "ID":
            assert out[-1] == runs[-1]
        assert len(out) <= len(runs) + len(shifts)
        gaps += len(shifts)
        moved += sum(1 for d in shifts if d)
    assert gaps > 1000 and moved > 300


@pytest.mark.parametrize("name,P,T,cigar,want", LC.HAND + LC.LONG, ids=[c[0] for c in LC.HAND + LC.LONG])
def test_hand_cases(name, P, T, cigar, want):
    runs = M.parse(cigar)
    assert M.check(P, T, runs) is None
    out, _ = M.left_align(P, T, runs)
    assert M.spell(out) == want
    assert M.check(P, T, out) is None and M.movable(P, T, out) == []


def test_movable_is_independent_of_the_rule():
    """the three stop rules, on CIGARs the rule has not seen"""
    P, T = b"CGAAAAAAGT", b"CGAAAAGT"
    assert M.movable(P, T, M.parse("6=2D2=")) == [1]
    assert M.movable(P, T, M.parse("2=2D6=")) == []            # the base before the gap differs from its last base
    assert M.movable(b"AAAAGT", b"AAGT", M.parse("1=2D3=")) == []  # the first run would go
    assert M.movable(b"CGAAAAAAAGT", b"CGAAAAGT", M.parse("2=1D1=2D5=")) == []  # would meet a gap of its op
    assert M.movable(b"CGTAAAGT", b"CGCAGT", M.parse("2=1X2D3=")) == []  # behind an X run


def test_entry_points_are_declared_and_exported():
    L = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfmash_hip.h")).read(), flags=re.S)
    assert re.search(r"\bwfm_left_align_runs\s*\(", text)
    assert "wfm_left_align_runs" in capi.EXPORTS and hasattr(L, "wfm_left_align_runs")
    assert C.sizeof(capi.LeftAlign) == 32 and capi.LeftAlign.bases_moved.offset == 16 and capi.LeftAlign.longest.offset == 24
    for name, value in (("WFM_LA_NOT_DONE", capi.WFM_LA_NOT_DONE), ("WFM_LA_SPANS", capi.WFM_LA_SPANS)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)u", text)
        assert m and int(m.group(1)) == value
    for name in ("wfmh_set_left_align", "wfmh_left_align_counts"):
        assert name in capi.HOST_EXPORTS and hasattr(L, name)


def test_switch_is_off_by_default_and_its_counts_are_zero():
    assert capi.left_align_counts() == (0, 0, 0, 0)
    capi.set_left_align(True)
    try:
        assert capi.left_align_counts() == (0, 0, 0, 0)
    finally:
        capi.set_left_align(False)


def _cli(args, cwd):
    return subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, text=True, timeout=60)


def test_cli_left_align_refused_with_m_before_any_device(tmp_path):
    r = _cli(["--left-align", "-m", "target.fa"], tmp_path)
    assert r.returncode == 1
    assert "--left-align" in r.stderr and "cannot be combined with -m" in r.stderr
    assert "device" not in r.stderr and r.stdout == ""


def test_cli_help_lists_the_flag(tmp_path):
    r = _cli(["--help"], tmp_path)
    assert r.returncode == 0 and "--left-align" in r.stderr + r.stdout
    head = open(os.path.join(ROOT, "wfmash_amd", "host", "main.cpp")).read().split("#include")[0]
    assert "--left-align" in head
