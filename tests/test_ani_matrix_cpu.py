"""CPU tests of the ANI table's boundary (no GPU): the new symbols are declared, listed and exported, the LDS limit equals the
header's, and the table's text is exactly what its definition says on hand-made counts."""
import os
import re

import numpy as np

from oracle import map_stats as MS
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "#query_group\ttarget_group\tquery_hashes\ttarget_hashes\tshared\tjaccard\tani\n"


def _header_text(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_new_symbols_are_declared_listed_and_exported():
    L = capi.load()
    hip, host = _header_text("wfmash_hip.h"), _header_text("wfmash_host.h")
    assert re.search(r"\bwfm_sketch_intersections\s*\(", hip)
    assert "wfm_sketch_intersections" in capi.EXPORTS and hasattr(L, "wfm_sketch_intersections")
    for name in ("wfmh_ani_matrix", "wfmh_ani_matrix_rows", "wfmh_free_ani_rows", "wfmh_set_ani_matrix", "wfmh_test_ani_tsv"):
        assert re.search(r"\b" + name + r"\s*\(", host), name
        assert name in capi.HOST_EXPORTS, name
        assert hasattr(L, name), name
    assert callable(capi.Handle.sketch_intersections) and callable(capi.ani_matrix)


def test_lds_limit_equals_the_header():
    m = re.search(r"#define\s+WFM_ISECT_LDS_MAX\s+(\d+)", open(os.path.join(ROOT, "include", "wfmash_hip.h")).read())
    assert m and capi.ISECT_LDS_MAX == int(m.group(1)) == 4096


def test_cli_refuses_before_it_opens_a_device(tmp_path):
    """--ani-only without a table to write, and a table together with -i (no map phase): status 1, a message, nothing written"""
    import subprocess
    cli = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
    fa = tmp_path / "x.fa"
    fa.write_text(">a#1#c\nACGTACGTAC\n")
    tsv = tmp_path / "t.tsv"
    r = subprocess.run([cli, "--ani-only", str(fa)], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--ani-only needs --ani-matrix" in r.stderr and r.stdout == b""
    r = subprocess.run([cli, "--ani-matrix", str(tsv), "-i", str(tmp_path / "m.paf"), str(fa)], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"cannot be combined with -i" in r.stderr and r.stdout == b""
    r = subprocess.run([cli, "--ani-matrix"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"missing value for --ani-matrix" in r.stderr
    assert not tsv.exists()
    r = subprocess.run([cli, "--help"], capture_output=True, timeout=60)
    assert b"--ani-matrix FILE" in r.stderr and b"--ani-only" in r.stderr


def _line(q, t, qn, tn, shared):
    """One row from the definition: jaccard = shared / the smaller sketch, ani = 1 - j2md(float32(jaccard), 21), zeros when nothing
    is shared or a sketch is empty; both as %.6f."""
    if shared and min(qn, tn):
        jac = shared / min(qn, tn)
        ani = 1.0 - float(MS.j2md(np.float32(jac), 21))
    else:
        jac = ani = 0.0
    return "%s\t%s\t%d\t%d\t%d\t%.6f\t%.6f\n" % (q, t, qn, tn, shared, jac, ani)


def test_formatter_writes_the_exact_text():
    rows = [
        ("HG01#1", "HG02#1", 4096, 4096, 3000),        # the usual row
        ("HG01#1", "other#1", 4096, 4096, 0),          # nothing shared: zeros
        ("HG02#2", "HG01#1", 4096, 680, 680),          # shared == the smaller sketch: ani 1.000000
        ("empty#1", "HG01#1", 0, 4096, 0),             # an empty sketch
        ("HG01#1", "empty#1", 4096, 0, 0),
        ("a#b#c#", "#", 1, 1, 1),                      # names with the delimiter in every place
        ("big", "big2", 20000, 4097, 1),               # one shared hash of thousands
    ]
    got = capi.host_ani_tsv(rows)
    assert got == HEADER + "".join(_line(*r) for r in rows)
    lines = got.split("\n")
    assert lines[1] == "HG01#1\tHG02#1\t4096\t4096\t3000\t0.732422\t%.6f" % (1.0 - float(MS.j2md(np.float32(3000 / 4096), 21)))
    assert lines[2] == "HG01#1\tother#1\t4096\t4096\t0\t0.000000\t0.000000"
    assert lines[3] == "HG02#2\tHG01#1\t4096\t680\t680\t1.000000\t1.000000"
    assert lines[4] == "empty#1\tHG01#1\t0\t4096\t0\t0.000000\t0.000000"
    assert lines[6] == "a#b#c#\t#\t1\t1\t1\t1.000000\t1.000000"
    assert 0.6 < float(lines[7].split("\t")[6]) < 0.7   # 1 of 4097: a Mash distance of about a third
    assert capi.host_ani_tsv([]) == HEADER
