"""CPU tests of the net across records: the brute force of tests/net_model.py against pieces written out by hand, and the boundary
(the header's symbols and the sizes of its structs as wfmash_amd/capi.py spells them)."""
import os
import re
import subprocess

import pytest

from tests import net_model as M
from tests.net_cases import HAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records(problems, n_bases):
    return [M.record(order, score, base, M.run_words(spec)) for order, score, base, spec in problems
            if not M.refused(base, M.run_words(spec), n_bases)]


@pytest.mark.parametrize("name,n_bases,problems,pieces,per", HAND, ids=[h[0] for h in HAND])
def test_model_on_hand_cases(name, n_bases, problems, pieces, per):
    got_pieces, got_per = M.net(_records(problems, n_bases))
    assert got_pieces == pieces
    orders = sorted(p[0] for p in problems)
    assert [r[0] for r in got_per] == orders
    assert [(r[1], r[3], r[4], r[5]) for r in got_per] == per
    # first: where the record's pieces begin in the list
    at = 0
    for r in got_per:
        assert r[2] == at
        at += r[3]
    assert at == len(pieces)


def test_model_is_a_set_function():
    name, n_bases, problems, pieces, per = HAND[2]
    for perm in ([2, 0, 1], [1, 2, 0], [2, 1, 0]):
        assert M.net(_records([problems[i] for i in perm], n_bases)) == M.net(_records(problems, n_bases))


def test_model_window_and_blocks():
    # a window that does not begin at 0 gives the same pieces, shifted
    recs = _records(HAND[0][2], 200)
    far = [{"order": r["order"], "score": r["score"], "blocks": [(t + (1 << 33), q, n) for t, q, n in r["blocks"]]} for r in recs]
    pieces, per = M.net(far, lo=(1 << 33) + 90)
    assert pieces == [(o, t + (1 << 33), q, n) for o, t, q, n in HAND[0][3]]
    # blocks: any number of I and D runs between two stretches, in any order; leading and trailing gaps belong to nobody
    spec = [(M.OP_D, 2), (M.OP_I, 3), (M.OP_M, 4), (M.OP_X, 1), (M.OP_I, 2), (M.OP_D, 7), (M.OP_I, 1), (M.OP_X, 2), (M.OP_M, 2), (M.OP_D, 3)]
    assert M.blocks_of_runs(100, M.run_words(spec)) == ([(102, 3, 5), (114, 11, 4)], 6)
    assert M.refused(0, [], 10) and M.refused(0, [0], 10) and M.refused(8, M.run_words([(M.OP_M, 3)]), 10)
    assert not M.refused(7, M.run_words([(M.OP_M, 3)]), 10) and not M.refused(10, M.run_words([(M.OP_I, 3)]), 10)


def test_boundary():
    import ctypes as C
    from wfmash_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfmash_hip.h")).read(), flags=re.S)
    L = capi.load()
    for name in ("wfm_net_create", "wfm_net_free", "wfm_net_add", "wfm_net_table", "wfm_net_export", "wfm_net_import", "wfm_net_counts",
                 "wfm_net_free_list"):
        assert re.search(r"\b" + name + r"\s*\(", text) and name in capi.EXPORTS and hasattr(L, name)
    assert capi.NET_PROB_DTYPE.itemsize == 32 and capi.NET_BLOCK_DTYPE.itemsize == 24
    assert capi.NET_REC_DTYPE.itemsize == 16 and capi.NET_CALL_DTYPE.itemsize == 48
    for name, value in (("WFM_NET_SCORE_EQ", capi.WFM_NET_SCORE_EQ), ("WFM_NET_SPANS", capi.WFM_NET_SPANS), ("WFM_NET_SCAN_BLOCK", capi.WFM_NET_SCAN_BLOCK)):
        m = re.search(r"#define\s+" + name + r"\s+(0x[0-9a-fA-F]+|\d+)u?", text)
        assert m and int(m.group(1), 0) == value
    assert M.SCORE_EQ == capi.WFM_NET_SCORE_EQ
    assert hasattr(capi, "Net") and hasattr(capi.Handle, "net")


# ---- the text side through the host library (chain_text.hpp's net_body), byte for byte against net_model.chain_text ----
def _rec(qname, qsize, qs, strand, tname, tsize, ts, cigar, t_offset):
    runs = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cigar)]
    return dict(qname=qname, qsize=qsize, qs=qs, qe=qs + sum(n for n, op in runs if op != "D"), strand=strand, tname=tname, tsize=tsize, ts=ts,
                te=ts + sum(n for n, op in runs if op != "I"), runs=runs, t_offset=t_offset)


TEXT_RECORDS = [
    # s1: one long block [200, 700) of few = columns (score 100).  s2, a - record (score 270), beats it on [300, 422), [422, 482) and
    # [487, 577) -- an insertion and a deletion of its own between them -- and cuts it in two.  s3 (score 255) loses all three of its
    # blocks to s2 but for the five bases of s2's deletion, where it beats s1: its chain begins inside its THIRD block, so tStart and
    # qStart move.  s4 lies on another sequence.  s5 (score 40) wins nothing.
    _rec("s1#1#chr1", 5000, 100, "+", "ref#1#chr1", 3000, 200, "50=400X50=", 0),
    _rec("s2#1#chr1", 4000, 500, "-", "ref#1#chr1", 3000, 300, "80=2X40=7I60=5D90=", 0),
    _rec("s3#1#chr1", 900, 0, "+", "ref#1#chr1", 3000, 310, "30=12D25=3I200=", 0),
    _rec("s4#1#chr2", 700, 10, "-", "ref#1#chr2", 800, 0, "15=1X15=", 3000),
    _rec("s5#1#chr1", 600, 20, "+", "ref#1#chr1", 3000, 320, "40=", 0),
]


def _spec(records):
    """the records and the pieces the model's net leaves them, as wfmh_test_chain_net_lines reads them"""
    recs = [M.record(i, M.SCORE_EQ, r["t_offset"] + r["ts"], [(n << 2) | "=XID".index(op) for n, op in r["runs"]]) for i, r in enumerate(records)]
    pieces, per = M.net(recs)
    lines = []
    for order, score, first, count, _, _ in per:
        r = records[order]
        lines.append("R\t%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d" % (r["qname"], r["qsize"], r["qs"], r["qe"], r["strand"], r["tname"], r["tsize"], r["t_offset"], score))
        lines += ["P\t%d\t%d\t%d" % (t, q, n) for _, t, q, n in pieces[first:first + count]]
    return "\n".join(lines) + "\n", pieces, per


def test_text_byte_for_byte():
    from tests import chain_model as CM
    from wfmash_amd import capi
    spec, pieces, per = _spec(TEXT_RECORDS)
    got = capi.host_chain_net_lines(spec)
    assert got == M.chain_text(TEXT_RECORDS)
    chains = CM.parse_chains(got)
    assert [c[0]["id"] for c in chains] == [1, 2, 3, 4] and per[4][3] == 0  # s5 won nothing: no chain, and the ids do not skip
    by_q = {c[0]["qname"]: c for c in chains}
    # s3's blocks [310, 340), [352, 377) and most of [377, 577) went to s2: what is left is [482, 487), 105 bases into the third block
    assert by_q["s3#1#chr1"][0]["tstart"] == 482 and by_q["s3#1#chr1"][0]["tend"] == 487 and by_q["s3#1#chr1"][0]["qstart"] == 30 + 25 + 3 + 105
    assert by_q["s3#1#chr1"][0]["score"] == 255 and by_q["s3#1#chr1"][1] == [(5, 0, 0)]
    # the - record's query side is counted on the reverse strand, as --chain counts it; its own gaps stay as they were
    assert by_q["s2#1#chr1"][0]["qstrand"] == "-" and by_q["s2#1#chr1"][0]["qstart"] == 4000 - (500 + 279) and by_q["s2#1#chr1"][0]["qend"] == 4000 - 500
    assert by_q["s2#1#chr1"][1] == [(122, 0, 7), (60, 5, 0), (90, 0, 0)]
    # the long record is cut in two, and both gaps are non-zero where s2 lay between
    assert by_q["s1#1#chr1"][1] == [(100, 277, 277), (123, 0, 0)]
    # single coverage: every base of the first side lies under at most one chain
    for name, size in (("ref#1#chr1", 3000), ("ref#1#chr2", 800)):
        for pos in range(0, size, 7):
            assert len(CM.lift_pos(got, name, pos)) <= 1


def test_text_refuses_a_bad_spec():
    from wfmash_amd import capi
    for spec in ("P\t1\t2\t3\n", "R\tq\t10\t0\t5\t+\tt\t10\t0\n", "R\tq\t10\t0\t5\t+\tt\t10\t0\t5\nP\t1\t2\n", "X\n"):
        with pytest.raises(capi.WfmError):
            capi.host_chain_net_lines(spec)
    assert capi.host_chain_net_lines("") == b""


def test_host_boundary():
    from wfmash_amd import capi
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfmash_host.h")).read(), flags=re.S)
    L = capi.load()
    for name in ("wfmh_set_chain_net", "wfmh_chain_net_counts", "wfmh_chain_net_paf", "wfmh_test_chain_net_lines"):
        assert re.search(r"\b" + name + r"\s*\(", host) and name in capi.HOST_EXPORTS and hasattr(L, name)
    capi.set_chain_net(None)
    assert capi.chain_net_counts() == (0, 0, 0, 0)
    import ctypes as C
    assert C.sizeof(capi.AlignParams) == 88


CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")


@pytest.mark.parametrize("args, message", [
    (["--chain-net", "x.net", "-m"], "--chain-net writes chains of alignments: it cannot be combined with -m"),
    (["--chain-net", "x.net", "--verify-paf", "x.paf"], "--chain-net belongs to the align phase: it cannot be combined with --verify-paf"),
    (["--chain-net", "x.net", "--chain", "x.chain", "--chain-swap"], "--chain-net cannot be combined with --chain-swap: nets on the query side are not done"),
    (["--chain-net", "x.net", "--chain-swap"], "--chain-net cannot be combined with --chain-swap: nets on the query side are not done"),
    (["--chain-net", "x.net", "--chain-paf", "x.paf", "--left-align"], "--chain-paf runs nothing else"),
    (["--chain-net"], "missing value for --chain-net"),
])
def test_cli_refused_combinations(args, message):
    r = subprocess.run(["timeout", "-k", "10", "60", CLI] + (args + ["t.fa"] if args != ["--chain-net"] else args), capture_output=True, text=True)
    assert r.returncode == 1 and message in r.stderr, (r.returncode, r.stderr)


def test_cli_help_names_the_switch():
    r = subprocess.run(["timeout", "-k", "10", "60", CLI, "--help"], capture_output=True, text=True)
    assert "--chain-net FILE" in r.stdout + r.stderr
