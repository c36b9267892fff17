"""External seeds (-K) and scaffold chain output (--scaffold-out) end to end on the GPU, on the reference's LPA test data
(tests/golden/LPA.subset.fa.gz): a -K run aligns exactly what -i aligns from the -K -m output, and the map path writes
the same mapping PAF with or without --scaffold-out."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FASTA = os.path.join(HERE, "golden", "LPA.subset.fa.gz")
CLI = os.path.join(os.path.dirname(HERE), "wfmash_amd", "wfmash-hip")
MAP_FLAGS = ["-p", "90", "-P", "50k", "-t", "8"]


def _cli(args, cwd, timeout=120):
    subprocess.check_call([CLI] + args, cwd=str(cwd), timeout=timeout)


@pytest.fixture(scope="module")
def mapped(tmp_path_factory):
    """the map path's mapping PAF of the fixture, with and without --scaffold-out"""
    d = tmp_path_factory.mktemp("seeds_gpu")
    m, m2, sc = str(d / "map.paf"), str(d / "map_sc.paf"), str(d / "scaffolds.paf")
    _cli(["-m"] + MAP_FLAGS + ["--out", m, FASTA], d)
    _cli(["-m"] + MAP_FLAGS + ["--scaffold-out", sc, "--out", m2, FASTA], d)
    return d, m, m2, sc


def test_seeds_align_like_align_only(mapped):
    d, m, _, _ = mapped
    km, kaln, ialn = str(d / "k_m.paf"), str(d / "k_aln.paf"), str(d / "i_aln.paf")
    _cli(["-m", "-K", m] + MAP_FLAGS + ["--out", km, FASTA], d)
    _cli(["-K", m] + MAP_FLAGS + ["--out", kaln, FASTA], d)
    _cli(["-i", km, "-t", "8", "--out", ialn, FASTA], d)
    seeds = open(km).read().splitlines()
    assert len(seeds) >= 100 and all(l.split("\t")[-1].startswith("st:Z:") for l in seeds)
    a, b = open(kaln).read(), open(ialn).read()
    assert a == b
    recs = a.splitlines()
    assert len(recs) >= 0.9 * len(seeds)
    assert all(any(x.startswith("cg:Z:") and len(x) > 5 for x in l.split("\t")) for l in recs)
    assert not [f for f in os.listdir(d) if f.startswith("wfmash-")]  # the hand-off file is removed


def test_scaffold_out_leaves_mappings_unchanged(mapped):
    _, m, m2, sc = mapped
    assert open(m).read() == open(m2).read()
    maps = [l.split("\t") for l in open(m).read().splitlines()]
    chains = [l.split("\t") for l in open(sc).read().splitlines()]
    assert chains
    for c in chains:
        assert len(c) == 15 and c[11] == "60" and c[12] == "tp:A:S" and c[13].startswith("id:f:") and c[14].startswith("kc:f:")
        qs, qe, ts, te, bl = int(c[2]), int(c[3]), int(c[7]), int(c[8]), int(c[10])
        assert c[4] in "+-" and int(c[1]) > 0 and int(c[6]) > 0 and qe > qs and te > ts
        assert bl >= 10000  # -S 10k (default)
        inside = [r for r in maps if r[0] == c[0] and r[5] == c[5] and r[4] == c[4] and int(r[2]) >= qs and int(r[3]) <= qe
                  and int(r[7]) >= ts and int(r[8]) <= te]
        assert inside, c


@pytest.mark.parametrize("extra", [["-i", "x.paf"], ["-W", "x.idx"], ["-I", "x.idx"]], ids=["i", "W", "I"])
def test_seeds_refuse_align_only_and_index(tmp_path, extra):
    seeds = tmp_path / "s.paf"
    seeds.write_text("")
    r = subprocess.run([CLI, "-K", str(seeds)] + extra + [FASTA], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-K" in r.stderr and "ERROR" in r.stderr
