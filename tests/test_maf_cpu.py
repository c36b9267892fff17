"""CPU tests of --maf: the brute-force model of the rule (tests/maf_model.py) against hand-written expectations, its inverse on seeded
random CIGARs, the - strand's start arithmetic on a case computed by hand, the text side (wfmash_amd/host/maf_text.hpp) through a
stand-alone program under ASan and UBSan, what the header and the Python layer state, and the command line's refusals, all without a GPU."""
import os
import random
import re
import subprocess

import pytest

from oracle import wflign_host as W
from tests import left_align_model as L
from tests import maf_model as M
from wfmash_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
P = L.parse


# ---- the rule, on literal bytes ----
def test_model_rows_by_hand():
    assert M.rows_of(b"ACGTA", b"ACGTA", P("5=")) == [(b"ACGTA", b"ACGTA")]
    assert M.rows_of(b"ACT", b"GTN", P("3X")) == [(b"ACT", b"GTN")]
    assert M.rows_of(b"ACGT", b"ACNGT", P("2=1I2=")) == [(b"AC-GT", b"ACNGT")]
    assert M.rows_of(b"ACTTGGA", b"ACCAGA", P("2=2I3D2=")) == [(b"AC--TTGGA", b"ACCA---GA")]
    # spelled from the runs, never from a comparison; lower case and other bytes stay
    assert M.rows_of(b"AAgG", b"AAT*", P("2X2=")) == [(b"AAgG", b"AAT*")]
    assert M.rows_of(b"", b"ACGN", P("4I")) == [(b"----", b"ACGN")]
    assert M.rows_of(b"TTGA", b"", P("4D")) == [(b"TTGA", b"----")]


def test_model_blocks_by_hand():
    # (p, t, psize, tsize, cols, eq, x)
    assert M.blocks_of(P("5=")) == [(0, 0, 5, 5, 5, 5, 0)]
    assert M.blocks_of(P("2=2I3D2=")) == [(0, 0, 7, 6, 9, 4, 0)]
    assert M.blocks_of(P("2X2=")) == [(0, 0, 4, 4, 4, 2, 2)]
    assert M.blocks_of(P("4I")) == [(0, 0, 0, 4, 4, 0, 0)] and M.blocks_of(P("4D")) == [(0, 0, 4, 0, 4, 0, 0)]


def test_model_split_by_hand():
    r = P("2=2I3D2=")  # a stretch of 5 gap bases
    for n in (1, 4, 5):
        assert M.blocks_of(r, n) == [(0, 0, 2, 2, 2, 2, 0), (5, 4, 2, 2, 2, 2, 0)]
        assert M.rows_of(b"ACTTGGA", b"ACCAGA", r, n) == [(b"AC", b"AC"), (b"GA", b"GA")]
    assert M.blocks_of(r, 6) == M.blocks_of(r, 0)
    # I and D runs of one stretch add up in either order, however many they are
    assert len(M.blocks_of(P("3=" + "1I1D" * 50 + "3="), 100)) == 2 and len(M.blocks_of(P("3=" + "1I1D" * 50 + "3="), 101)) == 1
    # a stretch below N stays inside its block, gaps and all
    assert M.blocks_of(P("3=1I2X9D4="), 9) == [(0, 0, 5, 6, 6, 3, 2), (14, 6, 4, 4, 4, 4, 0)]
    # two breaks with a one-column block between them
    assert M.blocks_of(P("5=9D1=4I5D7="), 6) == [(0, 0, 5, 5, 5, 5, 0), (14, 5, 1, 1, 1, 1, 0), (20, 10, 7, 7, 7, 7, 0)]
    # a break at the first or the last run yields no block on that side; a problem that is only a break has none
    assert M.blocks_of(P("6I4=1X"), 6) == [(0, 6, 5, 5, 5, 4, 1)]
    assert M.blocks_of(P("4=1X3I3D"), 6) == [(0, 0, 5, 5, 5, 4, 1)]
    assert M.blocks_of(P("3I3D"), 6) == [] and M.blocks_of(P("3I3D"), 7) == [(0, 0, 3, 3, 6, 0, 0)]


def test_model_call_layout():
    cases = [(b"ACTTGGA", b"ACCAGA", P("2=2I3D2=")), (b"AC", b"AC", []), (b"ACG", b"ACG", P("2=")), (b"ACG", b"ACT", P("2=1X"))]
    blocks, rows, per = M.call_of(cases, 5)
    assert rows == b"ACAC" b"GAGA" b"ACGACT"
    assert blocks == [(0, 0, 0, 0, 2, 2, 2, 2, 0), (4, 0, 5, 4, 2, 2, 2, 2, 0), (8, 3, 0, 0, 3, 3, 3, 2, 1)]
    assert per == [(0, 4, 0, 2), (M.NOT_DONE, 0, 2, 0), (M.SPANS, 1, 2, 0), (0, 2, 2, 1)]


# ---- the inverse ----
def _random_case(rng):
    """an aligned pair and its runs: = over equal bytes, X over different ones, gap runs between aligned ones, aligned at both ends"""
    runs, P_, T_ = [], bytearray(), bytearray()
    n = rng.randint(1, 40)
    for k in range(n):
        aligned = k % 2 == 0
        if aligned:
            for _ in range(rng.randint(1, 3)):
                op = "X" if runs and runs[-1][1] == "M" else "M" if runs and runs[-1][1] == "X" else rng.choice("MX")
                ln = rng.choice((1, 1, 2, 5, 30, 200))
                a = synth.random_dna(rng.getrandbits(30), ln)
                P_ += a
                T_ += a if op == "M" else a.translate(bytes.maketrans(b"ACGT", b"CGTA"))
                runs.append((ln, op))
        else:
            ops = rng.choice(("I", "D", "ID", "DI", "IDI"))
            for op in ops:
                ln = rng.choice((1, 2, 3, 4, 5, 6, 40, 99, 100, 101))
                if op == "I":
                    T_ += synth.random_dna(rng.getrandbits(30), ln)
                else:
                    P_ += synth.random_dna(rng.getrandbits(30), ln)
                runs.append((ln, op))
    if runs[-1][1] in "ID":
        P_ += b"A"
        T_ += b"A"
        runs.append((1, "M"))
    return bytes(P_), bytes(T_), runs


@pytest.mark.parametrize("split", [0, 1, 5, 100])
def test_inverse_round_trip(split):
    rng = random.Random(0x3AF0 + split)
    for _ in range(150):
        P_, T_, runs = _random_case(rng)
        assert not M.refused(P_, T_, runs)
        blocks = M.blocks_of(runs, split)
        rows = M.rows_of(P_, T_, runs, split)
        assert len(blocks) == len(rows) >= 1
        if split == 0:
            assert len(blocks) == 1
        kept = []
        for (p, t, psize, tsize, cols, eq, x), (rp, rt) in zip(blocks, rows):
            p2, t2, r2 = M.undo(rp, rt, eq)
            assert (p2, t2) == (P_[p:p + psize], T_[t:t + tsize]) and len(rp) == cols
            assert sum(n for n, op in r2 if op == "X") == x
            assert r2[0][1] in "MX" and r2[-1][1] in "MX"  # between breaks, and the problem begins and ends aligned
            kept.append(r2)
        # the blocks' runs are the problem's runs between the breaks, found here run by run: a second statement of the rule
        want, cur, k = [], [], 0
        while k < len(runs):
            e = k
            while e < len(runs) and runs[e][1] in "ID":
                e += 1
            if e > k and split >= 1 and sum(n for n, _ in runs[k:e]) >= split:
                want.append(cur)
                cur = []
            else:
                cur += runs[k:max(e, k + 1)]
            k = max(e, k + 1)
        want.append(cur)
        assert kept == [w for w in want if w]
        # and the bases between two blocks are the break's: at least `split` of them
        for (p, t, psize, tsize, *_), (p1, t1, *_) in zip(blocks, blocks[1:]):
            assert (p1 - p - psize) + (t1 - t - tsize) >= split >= 1


# ---- the file ----
def test_minus_strand_start_by_hand():
    """query of 30 bases, the line covers forward [10, 22) on -: T is the reverse complement of those 12 bases, and the source MAF counts
    on is the reverse complement of the WHOLE query, where that window begins at 30 - 22 = 8"""
    q = b"TTTTTTTTTT" b"ACGTACGGTTAA" b"CCCCCCCC"
    t = b"GG" + W.revcomp(q[10:22])[:5] + b"AAA" + W.revcomp(q[10:22])[5:] + b"GG"
    assert W.revcomp(q[10:22]) == b"TTAACCGTACGT"
    seqs = {"q": q, "t": t}
    r = dict(qname="q", qsize=30, qs=10, qe=22, strand="-", tname="t", tsize=len(t), ts=2, te=17, runs=P("5=3D7="))
    assert M.maf_text([r], seqs) == (b"##maf version=1\n"
                                     b"a score=12\ns t 2 15 + 19 TTAACAAACGTACGT\ns q 8 12 - 30 TTAAC---CGTACGT\n\n")
    # split at the deletion: the second block begins 5 bases further on the reverse-complemented source, at 8 + 5
    assert M.maf_text([r], seqs, split=3) == (b"##maf version=1\n"
                                              b"a score=5\ns t 2 5 + 19 TTAAC\ns q 8 5 - 30 TTAAC\n\n"
                                              b"a score=7\ns t 10 7 + 19 CGTACGT\ns q 13 7 - 30 CGTACGT\n\n")
    # the row is that strand: the reverse complement of the whole query, from the start the line names
    rcq = W.revcomp(q)
    assert rcq[8:8 + 12] == b"TTAACCGTACGT" and rcq[13:13 + 7] == b"CGTACGT"
    # and the same window on +
    r2 = dict(r, strand="+", runs=P("12="), te=14)
    seqs2 = {"q": q, "t": b"GG" + q[10:22] + b"GG"}
    assert M.maf_text([dict(r2, tsize=16)], seqs2, header=False) == b"a score=12\ns t 2 12 + 16 ACGTACGGTTAA\ns q 10 12 + 30 ACGTACGGTTAA\n\n"


def test_parse_maf_reads_what_maf_text_writes():
    rng = random.Random(0x3AF9)
    seqs, records = {}, []
    for k in range(20):
        P_, T_, runs = _random_case(rng)
        strand = "-" if k % 3 == 0 else "+"
        lead, trail = rng.randint(0, 9), rng.randint(0, 9)
        seqs["t%d" % k] = b"C" * lead + P_ + b"G" * trail
        seqs["q%d" % k] = b"A" * trail + (W.revcomp(T_) if strand == "-" else T_) + b"T" * lead
        records.append(dict(qname="q%d" % k, qsize=len(seqs["q%d" % k]), qs=trail, qe=trail + len(T_), strand=strand, tname="t%d" % k,
                            tsize=len(seqs["t%d" % k]), ts=lead, te=lead + len(P_), runs=runs))
    for split in (0, 5):
        text = M.maf_text(records, seqs, split)
        blocks = M.parse_maf(text)
        at = 0
        for r in records:
            P_, T_ = M.record_bases(seqs, r)
            shape = M.blocks_of(r["runs"], split)
            for (p, t, psize, tsize, cols, eq, x), b in zip(shape, blocks[at:at + len(shape)]):
                assert (b["tname"], b["tstart"], b["psize"], b["tstrand"], b["tsize"]) == (r["tname"], r["ts"] + p, psize, "+", r["tsize"])
                assert (b["qname"], b["qsize_row"], b["qstrand"], b["qsize"], b["score"]) == (r["qname"], tsize, r["strand"], r["qsize"], eq)
                p2, t2, _ = M.undo(b["row_p"], b["row_t"], eq)
                assert p2 == P_[p:p + psize] and t2 == T_[t:t + tsize]
                # the start names the row's bases on the strand the row is on
                src = W.revcomp(seqs[r["qname"]]) if r["strand"] == "-" else seqs[r["qname"]]
                assert src[b["qstart"]:b["qstart"] + tsize] == t2 and seqs[r["tname"]][b["tstart"]:b["tstart"] + psize] == p2
            at += len(shape)
        assert at == len(blocks)


def test_text_side_under_sanitizers(tmp_path):
    """scripts/micro/maf_check.cpp: maf_text.hpp driven by a program of its own, with its own main, under ASan and UBSan, run directly.
    The two runtimes are linked INTO the program (-static-libasan, -static-libubsan), so it starts whatever else the environment has
    loaders preload, and nothing is preloaded for it; no sanitizer goes near Python or the GPU"""
    exe = str(tmp_path / "maf_check")
    src = os.path.join(ROOT, "scripts", "micro", "maf_check.cpp")
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        src, "-o", exe], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    r = subprocess.run(["timeout", "-k", "10", "60", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "maf_check: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])


# ---- what the header and the Python layer state ----
def test_header_and_capi_agree():
    text = open(os.path.join(ROOT, "include", "wfmash_hip.h")).read()
    assert re.search(r"\bwfm_maf_rows\s*\(", text) and re.search(r"\bwfm_free_maf\s*\(", text)
    for name, value in (("WFM_MAF_NOT_DONE", capi.WFM_MAF_NOT_DONE), ("WFM_MAF_SPANS", capi.WFM_MAF_SPANS)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), text), name
    assert re.search(r"#define\s+WFM_MAF_SLICE\s+%d\b" % capi.WFM_MAF_SLICE, text)
    assert (capi.WFM_MAF_NOT_DONE, capi.WFM_MAF_SPANS) == (M.NOT_DONE, M.SPANS)
    import ctypes as C
    assert C.sizeof(capi.MafBlock) == 40 == capi.MAF_BLOCK_DTYPE.itemsize and C.sizeof(capi.MafCall) == 24
    assert [f[0] for f in capi.MafBlock._fields_] == list(capi.MAF_BLOCK_DTYPE.names) == ["off", "problem", "p", "t", "psize", "tsize", "cols", "eq", "x"]
    host = open(os.path.join(ROOT, "include", "wfmash_host.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, host) for n in ("wfmh_set_maf", "wfmh_maf_counts", "wfmh_maf_paf"))
    assert open(os.path.join(ROOT, "wfmash_amd", "host", "maf_text.hpp")).read().count(M.HEADER.decode().strip()) >= 1


# ---- the command line ----
def _cli(args):
    return subprocess.run(["timeout", "-k", "10", "60", CLI] + args, capture_output=True, text=True)


@pytest.mark.parametrize("args, message", [
    (["--maf-split", "50"], "--maf-split needs --maf FILE"),
    (["--maf-split", "10k", "-i", "x.paf"], "--maf-split needs --maf FILE"),
    (["--maf", "x.maf", "--maf-split", "7q"], "--maf-split expects a size such as 5000, 50k, 1m"),
    (["--maf-paf", "x.paf"], "--maf-paf needs --maf FILE"),
    (["--maf", "x.maf", "-m"], "--maf spells alignments: it cannot be combined with -m"),
    (["--maf", "x.maf", "--maf-split", "10k", "--verify-paf", "x.paf"], "--maf belongs to the align phase: it cannot be combined with --verify-paf"),
    (["--maf", "x.maf", "--maf-paf", "x.paf", "--left-align"], "--maf-paf runs nothing else"),
    (["--maf", "x.maf", "--chain-paf", "x.paf", "--chain", "x.chain"], "--chain-paf runs nothing else"),
    (["--maf"], "missing value for --maf"),
])
def test_cli_refused_combinations(args, message):
    r = _cli(args + ["t.fa"] if args != ["--maf"] else args)
    assert r.returncode == 1 and message in r.stderr, (r.returncode, r.stderr)


def test_cli_help_names_the_switches():
    r = _cli(["--help"])
    assert all(s in r.stdout + r.stderr for s in ("--maf FILE", "--maf-split N", "--maf-paf FILE"))
