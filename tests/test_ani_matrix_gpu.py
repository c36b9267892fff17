"""GPU tests of the group-by-group ANI table (wfmh_ani_matrix, --ani-matrix): its rows against the restatement of the estimate, the
estimate reproduced from the table, and the command line."""
import os
import subprocess

import numpy as np
import pytest

from oracle import map_ani as ANI
from oracle import map_pipeline as MP
from oracle import map_stats as MS
from wfmash_amd import capi
from tests.test_map_paf_gpu import _pangenome, _write_fasta

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wfmash_amd", "wfmash-hip")
HEADER = "#query_group\ttarget_group\tquery_hashes\ttarget_hashes\tshared\tjaccard\tani\n"


def _two_pointer(a, b):
    """the merge of map_stats.hpp:719-731: per value the smaller multiplicity, summed (tests/test_sketch_intersections_gpu.py holds
    this form against the loop itself)"""
    ua, ca = np.unique(a, return_counts=True)
    ub, cb = np.unique(b, return_counts=True)
    _, ia, ib = np.intersect1d(ua, ub, assume_unique=True, return_indices=True)
    return int(np.minimum(ca[ia], cb[ib]).sum())


@pytest.fixture(scope="module")
def pan(tmp_path_factory):
    """the pangenome of test_map_ani_gpu.py, and the table's rows restated: sketches from the restatement of StreamingMinHash, pooled
    per group, every ordered pair of different groups in ascending group order"""
    d = tmp_path_factory.mktemp("ani_matrix")
    seqs = _pangenome(51)
    fa = str(d / "pan.fa")
    _write_fasta(fa, seqs)
    names = [n for n, _ in seqs]
    groups = MP.ref_groups(names)
    prefix = {g: n[:n.rfind("#")] for g, n in zip(groups, names)}
    pooled = {}
    for g, (_, sq) in zip(groups, seqs):
        pooled[g] = ANI.pool(pooled.get(g, np.zeros(0, dtype=np.uint64)), ANI.minhash_sketch(sq))
    exp = []
    for q in sorted(pooled):
        for t in sorted(pooled):
            if q != t:
                exp.append((prefix[q], prefix[t], len(pooled[q]), len(pooled[t]), _two_pointer(pooled[q], pooled[t])))
    return fa, seqs, groups, exp, d


@pytest.fixture(scope="module")
def rows(gpu, pan):
    return capi.ani_matrix(gpu, pan[0])


def _tsv(rows):
    return HEADER + "".join("%s\t%s\t%d\t%d\t%d\t%.6f\t%.6f\n" % r for r in rows)


def test_rows_equal_the_restatement(pan, rows):
    exp = pan[3]
    assert len(exp) == 8 * 7 and len(rows) == len(exp)
    assert [r[:5] for r in rows] == exp
    for q, t, qn, tn, shared, jac, ani in rows:
        if shared == 0:
            assert jac == 0.0 and ani == 0.0
            continue
        assert jac == shared / min(qn, tn)
        assert ani == 1 - float(MS.j2md(np.float32(jac), 21))
    assert sum(1 for r in rows if r[4] == 0) >= 14                    # the unrelated sequence shares nothing with anybody
    assert any(r[2] < 1000 for r in rows)                             # the 700-base sequence's sketch is short
    assert max(r[6] for r in rows) > 0.95


@pytest.mark.parametrize("pctl,adj", [(50, -2.0), (25, 0.0)])
def test_the_table_reproduces_the_estimate(gpu, pan, rows, pctl, adj):
    fa, d = pan[0], pan[4]
    anis = sorted(r[6] for r in rows if r[4] > 0)
    idx = min(pctl * len(anis) // 100, len(anis) - 1)
    exp = min(1.0, max(0.0, anis[idx] + float(np.float32(adj)) / 100.0))
    P = capi.map_default_params(ani_percentile=pctl, ani_adjustment=adj)
    summ = capi.map_paf(gpu, fa, str(d / f"est{pctl}.paf"), params=P)
    assert summ.percentage_identity == np.float32(exp)
    assert 0.90 < summ.percentage_identity < 1.0


def test_multi_handle_call_and_text_form(gpu, pan, rows):
    """a list of handles is taken as one handle is; wfmh_ani_matrix writes the rows' text"""
    assert capi.ani_matrix([gpu], pan[0]) == rows
    out = str(pan[4] / "direct.tsv")
    capi.ani_matrix_tsv(gpu, pan[0], out)
    assert open(out).read() == _tsv(rows)


def test_set_ani_matrix_holds_for_one_map_call(gpu, pan, rows):
    """wfmh_set_ani_matrix: the next map call writes the table -- also with a fixed -p, which needs no sketch of its own -- and takes
    the setting with it; the mapping is the one without the table"""
    fa, d = pan[0], pan[4]
    P = capi.map_default_params(auto_pct_identity=0, percentage_identity=0.9)
    plain = str(d / "fixed_plain.paf")
    capi.map_paf(gpu, fa, plain, params=P)
    tsv, with_table, after = str(d / "set.tsv"), str(d / "fixed_table.paf"), str(d / "fixed_after.paf")
    capi.set_ani_matrix(tsv)
    capi.map_paf(gpu, fa, with_table, params=P)
    assert open(tsv).read() == _tsv(rows)
    os.unlink(tsv)
    capi.map_paf(gpu, fa, after, params=P)
    assert not os.path.exists(tsv)
    assert open(with_table, "rb").read() == open(plain, "rb").read() == open(after, "rb").read()
    assert os.path.getsize(plain) > 0


def test_cli_table_written_during_a_mapping_run(pan, rows):
    fa, d = pan[0], pan[4]
    tsv = str(d / "t.tsv")
    a = subprocess.run([CLI, "-m", "--ani-matrix", tsv, fa], capture_output=True, timeout=300)
    b = subprocess.run([CLI, "-m", fa], capture_output=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert open(tsv).read() == _tsv(rows)
    assert a.stdout == b.stdout and len(a.stdout.splitlines()) > 5


def test_cli_ani_only(pan, rows):
    fa, d = pan[0], pan[4]
    tsv = str(d / "only.tsv")
    r = subprocess.run([CLI, "--ani-only", "--ani-matrix", tsv, fa], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == b""
    assert open(tsv).read() == _tsv(rows)
    assert b"[wfmash::map]" not in r.stderr                          # no index, no mapping


def test_cli_refused_combinations(pan):
    fa, d = pan[0], pan[4]
    r = subprocess.run([CLI, "--ani-only", fa], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--ani-only needs --ani-matrix" in r.stderr and r.stdout == b""
    tsv = str(d / "refused.tsv")
    for flag in ("-i", "--align-paf"):
        r = subprocess.run([CLI, "--ani-matrix", tsv, flag, str(d / "none.paf"), fa], capture_output=True, timeout=60)
        assert r.returncode == 1 and b"--ani-matrix" in r.stderr and r.stdout == b""
    assert not os.path.exists(tsv)
