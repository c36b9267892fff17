"""--verify-optimal: every device call of the align driver -- main BiWFA problems, head and tail patches, late tails -- proves its scores optimal
with wfm_check_optimal before its results are used (GpuBatch::run, wfmash_amd/host/wflign_hip.cpp).  A small pangenome is made here -- 4
haplotypes of 12 kb at 1 - 6 % and one reverse-complemented -- with 18 mapping rows; the align phase runs in-process and through the CLI,
by host pointer and with resident sequences, and must write the bytes it writes without the switch."""
import os
import random
import re
import subprocess
import types

import pytest

from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
RC = bytes.maketrans(b"ACGT", b"TGCA")
SUMMARY = re.compile(r"\[wfmash::verify\] optimal: (\d+) problems checked, (\d+) failed, (\d+) skipped \(over the cell cap\), (\d+) cells")


def _make_case(d, seed=0x0B71, n_hap=4, L=12000, rows=18):
    rng = random.Random(seed)
    base = synth.random_dna(seed, L)
    seqs = {}
    for h in range(n_hap):
        seqs["hap%d#1#chr1" % h] = synth.mutate(base, [0.01, 0.03, 0.06, 0.02][h % 4], seed * 100 + h)
    seqs["hap9#1#chr1"] = synth.mutate(base, 0.04, seed * 100 + 9)[::-1].translate(RC)
    fa = os.path.join(d, "pan.fa")
    with open(fa, "w") as f:
        for name, s in seqs.items():
            f.write(">" + name + "\n")
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70].decode() + "\n")
    names = list(seqs)
    lines = []
    for chain in range(1, rows + 1):
        # (every third row against the reverse-complemented haplotype)
        qn, tn = ("hap9#1#chr1", rng.choice(names[:-1])) if chain % 3 == 0 else rng.sample(names[:-1], 2)
        ql, tl = len(seqs[qn]), len(seqs[tn])
        seg = rng.choice([1500, 4000, 9000])
        qs = rng.randrange(0, min(ql, tl) - seg - 600)
        qe = qs + seg
        rev = qn == "hap9#1#chr1"
        ts, te = (tl - qe, tl - qs) if rev else (qs, qe)
        ts = max(0, ts + rng.randrange(-60, 60))
        te = min(tl, te + rng.randrange(-60, 60))
        lines.append("\t".join(map(str, [qn, ql, qs, qe, "-" if rev else "+", tn, tl, ts, te, 100, seg, 30, "id:f:0.95", "kc:f:0.9", "ch:Z:%d.1.1" % chain])))
    paf = os.path.join(d, "map.paf")
    with open(paf, "w") as f:
        f.write("\n".join(lines) + "\n")
    return fa, paf


def _align(gpu, case, out, on, max_cells=0, **params):
    capi.set_verify_optimal(on, max_cells)
    try:
        capi.align_paf(gpu, case.fa, case.paf, out, params=params or None)
        return open(out, "rb").read(), capi.verify_optimal_counts()
    finally:
        capi.set_verify_optimal(False)


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows and the aligned PAF of a run without the check: made once, never changed"""
    d = str(tmp_path_factory.mktemp("verify_optimal"))
    fa, paf = _make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf)
    c.text, counts = _align(gpu, c, os.path.join(d, "plain.paf"), False)
    assert counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.records = len(c.text.decode().splitlines())
    assert c.records >= 15
    return c


def test_in_process(gpu, case):
    text, (checked, failed, skipped, cells) = _align(gpu, case, os.path.join(case.dir, "v.paf"), True)
    assert text == case.text
    assert failed == 0 and skipped == 0
    assert checked > case.records and cells > 0   # (patches count)


def test_in_process_with_resident_sequences(gpu, case):
    plain, counts0 = _align(gpu, case, os.path.join(case.dir, "r0.paf"), False, resident_sequences=1)
    text, (checked, failed, skipped, cells) = _align(gpu, case, os.path.join(case.dir, "r1.paf"), True, resident_sequences=1)
    assert counts0 == (0, 0, 0, 0)
    assert text == plain == case.text
    assert failed == 0 and skipped == 0 and checked > case.records and cells > 0


def _cli(args):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "120", CLI] + args, capture_output=True, text=True)


@pytest.mark.parametrize("extra", ([], ["--resident-seqs"], ["--verify"]), ids=("host_pointer", "resident", "with_verify"))
def test_cli(case, extra):
    out = os.path.join(case.dir, "cli%d.paf" % len("".join(extra)))
    r = _cli(["--verify-optimal", "-i", case.paf, "--out", out, case.fa] + extra)
    assert r.returncode == 0, r.stderr[-800:]
    m = SUMMARY.search(r.stderr)
    assert m, r.stderr[-800:]
    checked, failed, skipped, cells = map(int, m.groups())
    assert failed == 0 and skipped == 0 and checked > case.records and cells > 0
    assert "NOT OPTIMAL" not in r.stderr and "UNREACHED" not in r.stderr
    assert open(out, "rb").read() == case.text


def test_cli_without_the_flag_says_nothing(case):
    out = os.path.join(case.dir, "cli_plain.paf")
    r = _cli(["-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0 and "optimal" not in r.stderr
    assert open(out, "rb").read() == case.text


def test_cli_cell_cap_skips_everything(case):
    out = os.path.join(case.dir, "cli_cap.paf")
    r = _cli(["--verify-optimal", "--verify-optimal-cells", "1000", "-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0, r.stderr[-800:]
    m = SUMMARY.search(r.stderr)
    assert m, r.stderr[-800:]
    checked, failed, skipped, cells = map(int, m.groups())
    assert checked > case.records and (failed, skipped, cells) == (0, checked, 0)
    assert open(out, "rb").read() == case.text


def test_cli_refused_with_approximate_mapping(case):
    r = _cli(["-m", "--verify-optimal", case.fa])
    assert r.returncode == 1 and "--verify-optimal" in r.stderr and "-m" in r.stderr
