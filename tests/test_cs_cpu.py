"""CPU tests of --cs: the model of the cs grammar (tests/cs_model.py) on the example of minimap2's manual and against its own inverse,
the boundary of the new entry points, and the command line without a GPU."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

from tests import cs_model as CS
from tests import left_align_model as M
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")


def test_the_example_of_minimap2s_manual():
    #   CGATCGATAAATAGAGTAG---GAATAGCA
    #   ||||||   ||||||||||   |||| |||
    #   CGATCG---AATAGAGTAGGTCGAATtGCA
    P, T = b"CGATCGATAAATAGAGTAGGAATAGCA", b"CGATCGAATAGAGTAGGTCGAATTGCA"
    runs = M.parse("6=3D10=3I4=1X3=")
    assert CS.cs_of(P, T, runs, CS.SHORT) == b":6-ata:10+gtc:4*at:3"
    assert CS.cs_of(P, T, runs, CS.LONG) == b"=CGATCG-ata=AATAGAGTAG+gtc=GAAT*at=GCA"
    assert CS.decode(b":6-ata:10+gtc:4*at:3", P).upper() == T
    p2, t2 = CS.decode(b"=CGATCG-ata=AATAGAGTAG+gtc=GAAT*at=GCA")
    assert (p2.upper(), t2.upper()) == (P, T)


def test_spelled_from_the_runs_never_from_a_comparison():
    assert CS.cs_of(b"AAN", b"AAn", M.parse("1=2X"), CS.SHORT) == b":1*aa*nn"      # an X over equal bytes, N lower-cased, n left alone
    assert CS.cs_of(b"ACG", b"TTT", M.parse("3="), CS.LONG) == b"=ACG"              # an M over different bytes: the pattern's
    assert CS.cs_of(b"AC-", b"T", M.parse("1I3D"), CS.SHORT) == b"+t-ac-"           # a byte outside A..Z stays
    with pytest.raises(ValueError):
        CS.decode(b":3x", b"ACG")
    with pytest.raises(ValueError):
        CS.decode(b":2", b"ACG")  # covers 2 of 3


def _random_case(rng):
    runs, last = [], None
    for _ in range(rng.randint(1, 40)):
        op = rng.choice([o for o in "MXID" if o != last])
        runs.append((rng.choice([1, 2, 3, 9, 10, 11, 99, 100, 101, 1000]) if op == "M" else rng.randint(1, 12), op))
        last = op
    plen = sum(n for n, o in runs if o != "I")
    tlen = sum(n for n, o in runs if o != "D")
    P = bytes(rng.choice(b"ACGTN") for _ in range(plen))
    T = bytes(rng.choice(b"ACGTN") for _ in range(tlen))
    return P, T, runs


def test_decode_inverts_cs_of_on_random_runs():
    rng = random.Random(0xC5)
    for _ in range(300):
        P, T, runs = _random_case(rng)
        short, long_ = CS.cs_of(P, T, runs, CS.SHORT), CS.cs_of(P, T, runs, CS.LONG)
        # the text the short form gives back is the aligned text with the pattern's bases under the M runs: equal to T where the runs
        # are a valid CIGAR; here the M runs cover random bases, so hold it against that text
        want, p, t = [], 0, 0
        for n, op in runs:
            if op == "M":
                want.append(P[p:p + n])
            elif op != "D":
                want.append(T[t:t + n])
            p += n if op != "I" else 0
            t += n if op != "D" else 0
        want = b"".join(want)
        assert CS.same_bases(CS.decode(short, P), want)
        p2, t2 = CS.decode(long_)
        assert CS.same_bases(p2, P) and CS.same_bases(t2, want)
        # the lengths the issue's table gives
        assert len(short) == sum(1 + len(str(n)) if op == "M" else 3 * n if op == "X" else 1 + n for n, op in runs)
        assert len(long_) == sum(3 * n if op == "X" else 1 + n for n, op in runs)


def test_entry_points_are_declared_and_exported():
    L = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfmash_hip.h")).read(), flags=re.S)
    assert re.search(r"\bwfm_cs_strings\s*\(", text) and re.search(r"\bwfm_free_cs\s*\(", text)
    for name in ("wfm_cs_strings", "wfm_free_cs"):
        assert name in capi.EXPORTS and hasattr(L, name)
    assert C.sizeof(capi.Cs) == 24 and capi.Cs.off.offset == 8 and capi.Cs.len.offset == 16
    for name, value in (("WFM_CS_NOT_DONE", capi.WFM_CS_NOT_DONE), ("WFM_CS_SPANS", capi.WFM_CS_SPANS)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)u", text)
        assert m and int(m.group(1)) == value
    for name, value in (("WFM_CS_SHORT", capi.WFM_CS_SHORT), ("WFM_CS_LONG", capi.WFM_CS_LONG), ("WFM_CS_SLICE", capi.WFM_CS_SLICE)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value
    for name in ("wfmh_set_cs", "wfmh_cs_counts"):
        assert name in capi.HOST_EXPORTS and hasattr(L, name)


def test_switch_is_off_by_default_and_its_counts_are_zero():
    assert capi.cs_counts() == (0, 0, 0, 0)
    capi.set_cs(2)
    try:
        assert capi.cs_counts() == (0, 0, 0, 0)
    finally:
        capi.set_cs(0)


def _cli(args, cwd):
    return subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,needles", [
    (["--cs=foo", "target.fa"], ["--cs takes =short or =long", "foo"]),
    (["--cs", "-m", "target.fa"], ["--cs", "cannot be combined with -m"]),
    (["--cs=long", "--verify-paf", "x", "target.fa"], ["--cs", "cannot be combined with --verify-paf"]),
], ids=["bad_value", "with_m", "with_verify_paf"])
def test_cli_refusals_before_any_device(tmp_path, args, needles):
    r = _cli(args, tmp_path)
    assert r.returncode == 1
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and all(n in lines[0] for n in needles), r.stderr
    assert "device" not in r.stderr and r.stdout == ""


def test_cli_value_is_attached_so_a_file_name_is_never_eaten(tmp_path):
    """`--cs long -m`: `long` is the target, not the flag's value -- the refusal is the one of -m, which comes behind the target's"""
    r = _cli(["--cs", "long", "-m"], tmp_path)
    assert r.returncode == 1
    assert "--cs takes" not in r.stderr and "need a target FASTA" not in r.stderr and "cannot be combined with -m" in r.stderr


def test_cli_help_lists_the_flag(tmp_path):
    r = _cli(["--help"], tmp_path)
    assert r.returncode == 0 and "--cs[=short|=long]" in r.stderr + r.stdout
    head = open(os.path.join(ROOT, "wfmash_amd", "host", "main.cpp")).read().split("#include")[0]
    assert "--cs=long" in head
