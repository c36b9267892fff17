"""--transitive through the align driver on tests/golden/LPA.subset.fa.gz all-vs-all: the file held byte for byte against the fast NumPy form
of tests/trans_model.py (which tests/test_transitive_cpu.py holds against the brute force) applied to the records of the PAF just written."""
import gzip
import os
import subprocess
import types

import pytest

from tests import trans_model as TM
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
LPA = os.path.join(ROOT, "tests", "golden", "LPA.subset.fa.gz")


def _fasta(path):
    names, lengths = [], []
    for line in gzip.open(path, "rt"):
        if line.startswith(">"):
            names.append(line[1:].split()[0])
            lengths.append(0)
        else:
            lengths[-1] += len(line.strip())
    return names, lengths


def _align(handles, case, tag, depth=None, left=False):
    """one align run over the mapping rows; depth None: the switch is off.  (PAF bytes, file bytes or None, counts)"""
    out = os.path.join(case.dir, tag + ".paf")
    trans = os.path.join(case.dir, tag + ".tsv") if depth is not None else None
    capi.set_transitive(case.bed if trans else None, trans, depth if trans else 2)
    capi.set_left_align(left)
    try:
        if len(handles) == 1:
            capi.align_paf(handles[0], LPA, case.map, out)
        else:
            capi.align_paf_multi(handles, LPA, case.map, out)
        return open(out, "rb").read(), open(trans, "rb").read() if trans else None, capi.transitive_counts()
    finally:
        capi.set_transitive(None, None)
        capi.set_left_align(False)


def _model(case, paf_bytes, depth):
    lines = paf_bytes.decode().splitlines()
    fast = TM.Fast(TM.paf_records(lines, case.names, case.lengths))
    ivs, per, rounds = fast.closures([(s["gstart"], s["gend"]) for s in case.seeds], depth)
    text = TM.file_text(case.names, case.lengths, case.seeds, ivs)
    return text.encode(), (len(lines), text.count("\n"), rounds, case.skipped)


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the mapping rows of LPA all-vs-all, a BED of five 1 kb windows on the first sequence (and two lines to skip), a run with the
    switch off and one at depth 2: made once, never changed"""
    d = str(tmp_path_factory.mktemp("transitive"))
    c = types.SimpleNamespace(dir=d, map=os.path.join(d, "map.paf"), bed=os.path.join(d, "seeds.bed"))
    c.names, c.lengths = _fasta(LPA)
    subprocess.check_call(["timeout", "-k", "10", "300", CLI, "-m", "-p", "90", "-P", "50k", "-t", "8", "--out", c.map, LPA], cwd=d)
    first = c.names[0]
    step = (c.lengths[0] - 2000) // 5
    bed = "# five windows\n" + "".join("%s\t%d\t%d\tw%d\n" % (first, 500 + k * step, 1500 + k * step, k) for k in range(5)) + "nobody\t0\t10\n"
    open(c.bed, "w").write(bed)
    c.seeds, c.skipped = TM.parse_seeds(bed, c.names, c.lengths)
    assert len(c.seeds) == 5 and c.skipped == 2
    c.plain, none, counts = _align([gpu], c, "plain")
    assert none is None and counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.text, c.trans, c.counts = _align([gpu], c, "d2", depth=2)
    return c


def test_the_paf_does_not_change(case):
    assert case.text == case.plain and len(case.plain.splitlines()) >= 100


def test_depth_2_is_the_models(case):
    want, counts = _model(case, case.text, 2)
    assert case.trans == want
    assert case.counts == counts
    lines = case.trans.decode().splitlines()
    assert len(lines) > len(case.seeds)
    for s in case.seeds:  # every seed's own interval is in the file
        assert "%s\t%d\t%d\t%s\t%s\t%d\t%d" % (case.names[s["seq"]], s["start"], s["end"], s["name"], case.names[s["seq"]], s["start"], s["end"]) in lines
    assert len({ln.split("\t")[0] for ln in lines}) >= 3  # other sequences are reached


def test_depth_1_is_the_models(gpu, case):
    text, trans, counts = _align([gpu], case, "d1", depth=1)
    want, wc = _model(case, text, 1)
    assert text == case.plain and trans == want and counts == wc
    assert trans != case.trans


def test_with_left_align(gpu, case):
    text, trans, counts = _align([gpu], case, "la", depth=2, left=True)
    want, wc = _model(case, text, 2)
    assert text != case.plain  # the normalised runs are what the records hold
    assert trans == want and counts == wc


def test_two_handles_on_one_device(gpu, case):
    h2 = capi.Handle(0)
    try:
        text, trans, counts = _align([gpu, h2], case, "m", depth=2)
    finally:
        h2.close()
    assert text == case.plain and trans == case.trans and counts == case.counts


def test_transitive_paf_entry_point(gpu, case, tmp_path):
    """--transitive-paf on the PAF just written gives the file byte for byte, through the library and through the command line"""
    aligned = os.path.join(case.dir, "d2.paf")
    out = str(tmp_path / "paf.tsv")
    counts = capi.transitive_paf(gpu, LPA, aligned, case.bed, out)
    assert open(out, "rb").read() == case.trans and counts == case.counts
    out1 = str(tmp_path / "paf1.tsv")
    r = subprocess.run(["timeout", "-k", "10", "120", CLI, "--transitive-paf", aligned, "--transitive", case.bed, "--transitive-out", out1,
                        "--transitive-depth", "1", LPA], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out1, "rb").read() == _model(case, case.text, 1)[0]
    # a line whose query no FASTA has is skipped and counted; the others make the file of the PAF without it
    lines = case.text.decode().splitlines(True)
    odd = str(tmp_path / "odd.paf")
    open(odd, "w").write("nobody\t" + lines[0].split("\t", 1)[1] + "".join(lines[1:]))
    out2 = str(tmp_path / "odd.tsv")
    counts = capi.transitive_paf(gpu, LPA, odd, case.bed, out2)
    want, wc = _model(case, "".join(lines[1:]).encode(), 2)
    assert open(out2, "rb").read() == want and counts == wc
