"""CPU tests of external seeds (-K, wfmh_seed_paf; host/external_seeds.cpp) and of the scaffold chain output
(--scaffold-out): the seeder's parsing rules on hand-written PAF lines, its filters against the reference's own
filter code (oracle/_ref/libref_filter.so), and the scaffold lines on a constructed case."""
import collections
import os
import subprocess

import pytest

from oracle import pyfilter
from tests import filter_cases as FC
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
LEN = dict(FC.NAMES)


@pytest.fixture(scope="module")
def fai(tmp_path_factory):
    return FC.write_fai(str(tmp_path_factory.mktemp("seeds_fai")))


def _seed_line(q, qs, qe, strand, t, ts, te, *tags, qlen=None):
    return "\t".join([q, str(LEN[q] if qlen is None else qlen), str(qs), str(qe), strand, t, str(LEN.get(t, 1000)), str(ts), str(te),
                      "0", str(te - ts), "255"] + list(tags))


def _run(fai, tmp_path, lines, tag="s", **over):
    seeds, out = str(tmp_path / f"{tag}.seeds.paf"), str(tmp_path / f"{tag}.out.paf")
    with open(seeds, "w") as f:
        f.write("".join(l + "\n" for l in lines))
    over.setdefault("auto_pct_identity", 0)
    over.setdefault("percentage_identity", 0.9)
    s = capi.seed_paf(fai, seeds, out, params=capi.map_default_params(**over))
    return s, [l.split("\t") for l in open(out).read().splitlines()]


def test_parsing_rules(fai, tmp_path):
    lines = [
        "A#1#c1\t300000\t0\t1000\t+\tB#1#c1\t310000\t0\t1000\t0\t1000",              # 11 fields: skipped
        _seed_line("A#1#c1", 0, 1000, "*", "B#1#c1", 0, 1000),                          # bad strand: skipped
        _seed_line("A#1#c1", 0, 1000, "+", "nowhere", 0, 1000),                         # unknown target: skipped
        _seed_line("A#1#c1", 5000, 5500, "+", "B#1#c1", 7000, 8000),                    # no tag: 0.9; end from the target span
        _seed_line("A#1#c1", 1000, 2000, "-", "C#1#c1", 3000, 4000, "dv:f:0.05"),       # 0.95
        _seed_line("A#1#c1", 3000, 4000, "+", "B#1#c1", 10000, 11000, "id:f:0.97", "cg:Z:500=1X499="),
        _seed_line("A#1#c1", 20000, 21000, "+", "B#1#c1", 30000, 31000, "dv:f:0.1", "id:f:0.8"),   # the later tag wins
        _seed_line("A#1#c1", 22000, 23000, "+", "B#1#c1", 32000, 33000, "id:f:0.8", "dv:f:0.02"),
        _seed_line("B#1#c2", 700, 900, "+", "A#1#c1", 100, 300, "id:f:1"),              # identity 1: MAPQ 255
        _seed_line("B#1#c2", 100, 200, "+", "A#2#c1", 100, 200, qlen=0),                # length 0: the id manager's
    ]
    s, rec = _run(fai, tmp_path, lines, filter_mode=3)
    assert s.l2_mappings == 7 and s.written == 7 and s.queries == 2
    # by query name, then by query start
    assert [(r[0], int(r[2])) for r in rec] == [("A#1#c1", 1000), ("A#1#c1", 3000), ("A#1#c1", 5000), ("A#1#c1", 20000),
                                                 ("A#1#c1", 22000), ("B#1#c2", 100), ("B#1#c2", 700)]
    by = {(r[0], int(r[2])): r for r in rec}
    r = by[("A#1#c1", 5000)]
    assert r[1:12] == ["300000", "5000", "6000", "+", "B#1#c1", "310000", "7000", "8000", "0", "1000", "10"]
    assert r[12:14] == ["id:f:0.9", "kc:f:1"] and r[14] == "ch:Z:" + r[14][5:] and r[-1] == "st:Z:"
    assert by[("A#1#c1", 1000)][4] == "-" and by[("A#1#c1", 1000)][12] == "id:f:0.95"
    r = by[("A#1#c1", 3000)]
    assert r[12] == "id:f:0.97" and "cg:Z:500=1X499=" in r and r.index("cg:Z:500=1X499=") == 15
    assert by[("A#1#c1", 20000)][12] == "id:f:0.8" and by[("A#1#c1", 22000)][12] == "id:f:0.98"
    assert by[("B#1#c2", 700)][11] == "255" and by[("B#1#c2", 700)][12] == "id:f:1"
    assert by[("B#1#c2", 100)][1] == "50000"
    assert all(len(r) >= 15 and r[14].startswith("ch:Z:") and r[14].endswith(".1.1") for r in rec)
    assert not any(x.startswith("cg:Z:") for r in rec if r[2] != "3000" for x in r)
    # -M: no chain tag
    _, rec = _run(fai, tmp_path, lines, tag="nomerge", filter_mode=3, merge_mappings=0)
    assert len(rec) == 7 and not any(x.startswith("ch:Z:") for r in rec for x in r)


def test_scaffold_tag_and_empty_input(fai, tmp_path):
    # one long seed (a scaffold on its own) and a short one beside it on the diagonal
    lines = [_seed_line("A#1#c1", 10000, 16000, "+", "B#1#c1", 20000, 26000),
             _seed_line("A#1#c1", 17000, 18000, "+", "B#1#c1", 27000, 28000)]
    _, rec = _run(fai, tmp_path, lines, scaffold_min_length=5000)
    assert [r[-1] for r in rec] == ["st:Z:scaffold", "st:Z:rescued"]
    s, rec = _run(fai, tmp_path, ["garbage"], tag="empty")
    assert rec == [] and s.written == 0


def _boundary_check(m):
    """MappingOutput::mappingBoundarySanityCheck, applied before the rows become seeds: the oracle's branch runs it, the seeder does not"""
    m = m.copy()
    for i in range(len(m)):
        tl = FC.NAMES[m["refSeqId"][i]][1]
        if m["refStartPos"][i] + m["blockLength"][i] >= tl:
            m["blockLength"][i] = tl - 1 - m["refStartPos"][i]
    return m


def _to_seeds(m, query):
    qlen = LEN[query]
    out = []
    for r in m:
        q0, bl = int(r["queryStartPos"]), int(r["blockLength"])
        if q0 + bl >= qlen:
            bl = qlen - q0
        t0 = int(r["refStartPos"])
        out.append(_seed_line(query, q0, q0 + bl, "-" if r["flags"] & 1 else "+", FC.NAMES[r["refSeqId"]][0], t0, t0 + bl,
                              f"id:f:{r['nucIdentity'] / 10000:.4f}"))
    return out


def _as_oracle_input(m, query):
    """the values the seeder assigns: kc 1, conserved 0, n_merged 1, the tag's identity, the query end clipped as above"""
    m = m.copy()
    qlen = LEN[query]
    for i in range(len(m)):
        if m["queryStartPos"][i] + m["blockLength"][i] >= qlen:
            m["blockLength"][i] = qlen - m["queryStartPos"][i]
    m["kmerComplexity"] = 100
    m["conservedSketches"] = 0
    m["n_merged"] = 1
    m["flags"] &= 1
    return m


def _key(fields):
    return tuple(fields[:12]) + tuple(x for x in fields[12:] if x.startswith("id:f:"))


PARITY = [("defaults", {}), ("n1", {"num_mappings_for_segment": 1}), ("n3", {"num_mappings_for_segment": 3}),
          ("filter_none", {"filter_mode": 3}), ("no_scaffold_mass", {"scaffold_min_length": 0}),
          ("small_jump", {"scaffold_gap": 20000, "scaffold_min_length": 15000})]


@pytest.mark.skipif(not pyfilter.have_ref(), reason="oracle/_ref/libref_filter.so not built (needs the reference tree)")
@pytest.mark.parametrize("name,over", PARITY, ids=[p[0] for p in PARITY])
@pytest.mark.parametrize("seed", [1, 2, 6])
def test_filters_match_reference(fai, tmp_path, name, over, seed):
    """seed_paf against the reference's own filterByGroup + filterByScaffolds (the oracle's no-merge branch of 'subset'; sparsify is a
    no-op at -x 1).  The seeder skips the scaffold filter with -f or -S 0; the oracle's branch is told the same by -j 0.  The oracle's
    branch chains first, which reorders its vector; no tie in these cases' sweeps depends on that order, so the seeds are written in
    the cases' own order and compared as multisets per query, columns 1-12 and id:f."""
    query = "A#1#c1" if seed != 2 else "C#1#c1"
    m = _boundary_check(FC.make_mappings(name, query, seed, {}))
    seeds = _to_seeds(m, query)
    _, got = _run(fai, tmp_path, seeds, tag=name, auto_pct_identity=0, **over)
    ref_over = dict(over, merge_mappings=0)
    if over.get("filter_mode") == 3 or over.get("scaffold_min_length", 1) == 0:
        ref_over["scaffold_gap"] = 0
    ref = pyfilter.ref_filter("subset", _as_oracle_input(m, query), fai, query, capi.map_default_params(**ref_over))
    want = [l.split("\t") for l in ref.splitlines()]
    assert collections.Counter(map(_key, got)) == collections.Counter(map(_key, want))
    assert len(got) >= 5
    if name == "filter_none":
        assert len(got) == len(seeds)
    elif name == "n1":
        assert len(got) < len(seeds)


def test_scaffold_out_constructed(fai, tmp_path):
    # a syntenic run of 40 seeds on B#1#c1 plus decoys on C#1#c1 along the anti-diagonal (they never chain)
    lines = [_seed_line("A#1#c1", i * 1000, i * 1000 + 1000, "+", "B#1#c1", 5000 + i * 1000, 6000 + i * 1000) for i in range(40)]
    lines += [_seed_line("A#1#c1", 100000 + k * 20000, 101000 + k * 20000, "+", "C#1#c1", 250000 - k * 30000, 251000 - k * 30000, "id:f:0.95")
              for k in range(6)]
    sc = str(tmp_path / "scaffolds.paf")
    s, rec = _run(fai, tmp_path, lines, tag="syn", scaffold_out=sc)
    assert open(sc).read() == "A#1#c1\t300000\t0\t40000\t+\tB#1#c1\t310000\t5000\t45000\t0\t40000\t60\ttp:A:S\tid:f:0.9\tkc:f:1\n"
    assert len(rec) == 40 and {r[5] for r in rec} == {"B#1#c1"}
    # the same through the command line (-K -m is host only)
    seeds = str(tmp_path / "syn.seeds.paf")
    out, sc2 = str(tmp_path / "cli.paf"), str(tmp_path / "cli.scaffolds.paf")
    subprocess.check_call([CLI, "-m", "-p", "90", "-K", seeds, "--scaffold-out", sc2, "--out", out, fai], cwd=str(tmp_path), timeout=60)
    assert open(sc2).read() == open(sc).read()
    assert open(out).read() == open(str(tmp_path / "syn.out.paf")).read()
    # -S longer than the query: no scaffold, an empty file (and nothing survives the scaffold filter)
    sc3 = str(tmp_path / "none.paf")
    _, rec = _run(fai, tmp_path, lines, tag="big", scaffold_out=sc3, scaffold_min_length=400000)
    assert os.path.exists(sc3) and open(sc3).read() == "" and rec == []


def test_align_row_parser_reads_seed_records():
    """an -K record (cg:Z and st:Z after ch:Z) is a row of the align phase like the mapper's: tokens 12 and 14 are what it reads"""
    line = "A#1#c1\t300000\t3000\t4000\t+\tB#1#c1\t310000\t10000\t11000\t0\t1000\t15\tid:f:0.97\tkc:f:1\tch:Z:3.1.1\tcg:Z:1000=\tst:Z:"
    r = capi.host_cigar_fn("parse_row", line, i0=0, i1=0).split(",")
    assert r == ["A#1#c1", "3000", "4000", "+", "B#1#c1", "10000", "11000", "0.97", "3", "1", "1"]


def test_no_scaffold_output_without_request(fai, tmp_path):
    """the map path's filter test hook is unchanged by the new parameter block field (NULL = nothing kept)"""
    m = FC.make_mappings("defaults", "A#1#c1", 1, {})
    assert capi.host_filter("subset", m, fai, "A#1#c1", capi.map_default_params()) == \
        capi.host_filter("subset", m, fai, "A#1#c1", capi.map_default_params(scaffold_out=str(fai) + ".unused"))
    assert not os.path.exists(str(fai) + ".unused")
