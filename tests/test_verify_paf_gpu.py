"""--verify and --verify-paf: every finished PAF line held against its bases on the device (wfmash_amd/host/verify_paf.cpp on top of
wfm_check_runs).  A small pangenome is made here -- 4 haplotypes of 40 kb and one reverse-complemented -- with about 24 mapping rows;
the align phase runs with the in-run check on and off, and the file it wrote is verified as it stands and with three lines corrupted."""
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


def _write_fasta(path, seqs, width=70):
    with open(path, "w") as f:
        for name, s in seqs.items():
            f.write(">" + name + "\n")
            s = s.decode()
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + "\n")


def _make_case(d, seed=0x5EED, n_hap=4, L=40000, rows=24):
    rng = random.Random(seed)
    base = synth.random_dna(seed, L)
    seqs = {}
    for h in range(n_hap):
        s = synth.mutate(base, rng.choice([0.01, 0.03, 0.06]), seed * 100 + h)
        if h == 1:  # lower case and IUPAC letters: the verifier must normalise its windows as the driver does
            b = bytearray(s)
            b[5000:5200] = bytes(b[5000:5200]).lower()
            b[9000:9005] = b"RYKMN"
            s = bytes(b)
        seqs["hap%d#1#chr1" % h] = s
    seqs["hap9#1#chr1"] = synth.mutate(base, 0.04, seed * 100 + 9)[::-1].translate(RC)
    fa = os.path.join(d, "pan.fa")
    _write_fasta(fa, seqs)
    names = list(seqs)
    lines = []
    for chain in range(1, rows + 1):
        # (every third row against the reverse-complemented haplotype: '-' lines are needed below)
        qn, tn = ("hap9#1#chr1", rng.choice(names[:-1])) if chain % 3 == 0 else rng.sample(names, 2)
        ql, tl = len(seqs[qn]), len(seqs[tn])
        seg = rng.choice([1500, 4000, 9000])
        qs = rng.randrange(0, min(ql, tl) - seg - 600)
        qe = qs + seg
        rev = (qn == "hap9#1#chr1") != (tn == "hap9#1#chr1")
        ts, te = (tl - qe, tl - qs) if rev else (qs, qe)
        ts = max(0, ts + rng.randrange(-60, 60))
        te = min(tl, te + rng.randrange(-60, 60))
        lines.append("\t".join(map(str, [qn, ql, qs, qe, "-" if rev else "+", tn, tl, ts, te, 100, seg, 30, "id:f:0.95", "kc:f:0.9", "ch:Z:%d.1.1" % chain])))
    paf = os.path.join(d, "map.paf")
    with open(paf, "w") as f:
        f.write("\n".join(lines) + "\n")
    return fa, paf


def _align(gpu, case, out, verify, **params):
    capi.set_verify(verify)
    try:
        capi.align_paf(gpu, case.fa, case.paf, out, params=params or None)
        return open(out, "rb").read(), capi.verify_counts()
    finally:
        capi.set_verify(False)


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows and the aligned PAF of a run without the check: made once, never changed"""
    d = str(tmp_path_factory.mktemp("verify"))
    fa, paf = _make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, good=os.path.join(d, "good.paf"))
    c.text, counts = _align(gpu, c, c.good, False)
    assert counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20 and all("cg:Z:" in l for l in c.lines)
    return c


def test_in_run_verify_leaves_the_output_alone(gpu, case):
    text, (checked, failed, unverifiable, bases) = _align(gpu, case, os.path.join(case.dir, "v.paf"), True)
    assert text == case.text
    assert (checked, failed, unverifiable) == (len(case.lines), 0, 0)
    # every = and X base of every line was compared
    want = sum(int(n) for l in case.lines for n, op in re.findall(r"(\d+)([=XID])", l.split("cg:Z:")[1].split("\t")[0]) if op in "=X")
    assert bases == want


def test_in_run_verify_with_resident_sequences(gpu, case):
    plain, counts0 = _align(gpu, case, os.path.join(case.dir, "r0.paf"), False, resident_sequences=1)
    text, (checked, failed, unverifiable, _) = _align(gpu, case, os.path.join(case.dir, "r1.paf"), True, resident_sequences=1)
    assert counts0 == (0, 0, 0, 0)
    assert text == plain == case.text
    assert (checked, failed, unverifiable) == (len(case.lines), 0, 0)


def test_verify_paf_on_the_output(gpu, case):
    checked, failed, unverifiable, bases = capi.verify_paf(gpu, case.fa, case.good)
    assert (checked, failed, unverifiable) == (len(case.lines), 0, 0) and bases > 0


def _record(line):
    f = line.split("\t")
    return "%s %s-%s %s %s %s-%s" % (f[0], f[2], f[3], f[4], f[5], f[7], f[8])


def _corrupt(case):
    """a copy of the aligned PAF with an =/X pair swapped in one line, ts shifted by one in another, one count of a '-' line changed
    by one, and the cg:Z: tag of a fourth line removed; returns (path, the three records that must fail)"""
    lines = list(case.lines)
    swap = next(i for i, l in enumerate(lines) if re.search(r"\d+=\d+X", l.split("cg:Z:")[1]))
    minus = next(i for i, l in enumerate(lines) if l.split("\t")[4] == "-" and i != swap)
    shift = next(i for i in range(len(lines)) if i not in (swap, minus))
    drop = next(i for i in range(len(lines)) if i not in (swap, minus, shift))
    head, cg = lines[swap].split("cg:Z:")
    lines[swap] = head + "cg:Z:" + re.sub(r"(\d+)=(\d+)X", r"\1X\2=", cg, count=1)
    f = lines[shift].split("\t")
    f[7] = str(int(f[7]) + 1)
    lines[shift] = "\t".join(f)
    head, cg = lines[minus].split("cg:Z:")
    lines[minus] = head + "cg:Z:" + re.sub(r"(\d+)=", lambda m: "%d=" % (int(m.group(1)) + 1), cg, count=1)
    lines[drop] = "\t".join(x for x in lines[drop].split("\t") if not x.startswith("cg:Z:"))
    path = os.path.join(case.dir, "bad.paf")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path, [_record(lines[i]) for i in (swap, shift, minus)]


def test_verify_paf_on_a_corrupted_copy(gpu, case, capfd):
    path, records = _corrupt(case)
    capfd.readouterr()
    checked, failed, unverifiable, _ = capi.verify_paf(gpu, case.fa, path)
    err = capfd.readouterr().err
    assert (checked, failed, unverifiable) == (len(case.lines) - 1, 3, 1)
    reported = [l for l in err.splitlines() if l.startswith("[wfmash::verify] FAILED")]
    assert len(reported) == 3
    for rec in records:
        assert any(rec in l for l in reported), (rec, reported)
    # the swapped pair is a base error with a position, the other two are span errors
    assert sum("X_EQUAL" in l or "M_DIFFERS" in l for l in reported) >= 1 and sum("SPANS" in l for l in reported) == 2
    assert sum("first offending base" in l for l in reported) >= 1


def _cli(args):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "120", CLI] + args, capture_output=True, text=True)


def test_cli_verify_paf(case):
    r = _cli(["--verify-paf", case.good, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert "%d lines checked, 0 failed, 0 unverifiable" % len(case.lines) in r.stderr
    path, records = _corrupt(case)
    r = _cli(["--verify-paf", path, case.fa])
    assert r.returncode == 3, r.stderr[-500:]
    assert all(rec in r.stderr for rec in records)
    assert r.stdout == ""


def test_cli_verify_in_an_align_run(case):
    out = os.path.join(case.dir, "cli.paf")
    r = _cli(["--verify", "-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert "[wfmash::verify] %d lines checked, 0 failed, 0 unverifiable" % len(case.lines) in r.stderr
    assert open(out, "rb").read() == case.text


def test_cli_verify_refused_with_sam(case):
    r = _cli(["--verify", "-a", "-i", case.paf, case.fa])
    assert r.returncode == 1 and "--verify" in r.stderr and "SAM" in r.stderr
