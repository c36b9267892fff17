"""CPU tests of --chain: the brute-force model of a chain (tests/chain_model.py) against hand-written expectations for each rule, the
text side (the two sides' coordinates, the flags, the writer's ids) through its test hook against the model byte for byte, a ten-line
liftOver through the model's files, and the command line's refusals, all without a GPU."""
import os
import random
import subprocess

import pytest

from tests import chain_model as M
from tests import lift_model as LM
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
P = LM.parse


def one(cigar, flags=0):
    blocks, per = M.chain_problems([(P(cigar), flags)])
    assert per[0][0] == 0 and per[0][2] == 0 and per[0][3] == len(blocks)
    return blocks, per[0][4:]


def test_model_rules():
    # a D run between two blocks; the last block has no gap behind it
    assert one("4=3D4=") == ([(4, 3, 0, 4), (4, 0, 0, 4)], (0, 0, 0, 0, 8, 0))
    # I and D runs between two blocks add up, in either order
    assert one("4=2I3D4=")[0][0] == (4, 3, 2, 4) and one("4=3D2I4=")[0][0] == (4, 3, 2, 4)
    assert one("5=" + "1I1D" * 10000 + "5=")[0] == [(5, 10000, 10000, 5), (5, 0, 0, 5)]
    # gaps before the first and behind the last block are the lead and the trail, (dt, dq) each
    assert one("2I5=2D") == ([(5, 0, 0, 5)], (0, 2, 2, 0, 5, 0))
    # = and X runs are one block; eq counts the = columns
    assert one("3=2X4=") == ([(9, 0, 0, 7)], (0, 0, 0, 0, 7, 2))
    assert one("1=1X1=1X") == ([(4, 0, 0, 2)], (0, 0, 0, 0, 2, 2))
    # gap runs only: no block, everything leads
    assert one("2I3D1I") == ([], (3, 3, 0, 0, 0, 0))
    # refused: no runs, an empty run, a span beyond 32 bits (never expanded)
    wide = [((1 << 30) - 1, "I")] * 4 + [(4, "I")]
    blocks, per = M.chain_problems([([], 0), (P("3=0D2="), 3), (wide, 0), (P("2="), 1)])
    assert blocks == [(2, 0, 0, 2)] and [p[0] for p in per] == [2, 2, 2, 0] and per[2] == (2, 5, 0, 0, 0, 0, 0, 0, 0, 0) and per[3][2:4] == (0, 1)


def test_model_flags():
    c = "1I3=1D2I1X4D2=5D"  # 3= (1D, 2I) 1X (4D, 0I) 2=, lead 1I, trail 5D
    assert one(c, 0) == ([(3, 1, 2, 3), (1, 4, 0, 0), (2, 0, 0, 2)], (0, 1, 5, 0, 5, 1))
    assert one(c, M.SWAP) == ([(3, 2, 1, 3), (1, 0, 4, 0), (2, 0, 0, 2)], (1, 0, 0, 5, 5, 1))
    assert one(c, M.REVERSE) == ([(2, 4, 0, 2), (1, 1, 2, 0), (3, 0, 0, 3)], (5, 0, 0, 1, 5, 1))
    assert one(c, M.SWAP | M.REVERSE) == ([(2, 0, 4, 2), (1, 2, 1, 0), (3, 0, 0, 3)], (0, 5, 1, 0, 5, 1))


def _random_runs(rng, n_max=30):
    runs, last = [], None
    for _ in range(rng.randrange(1, n_max)):
        op = rng.choice([o for o in "=XID" if o != last])
        runs.append((rng.randrange(1, 9), op))
        last = op
    return runs


def test_model_reverse_and_swap_are_involutions():
    rng = random.Random(0xC4A1)
    for _ in range(300):
        shape = M.plain(_random_runs(rng))
        for f in (M.REVERSE, M.SWAP, M.SWAP | M.REVERSE):
            assert M.flagged(M.flagged(shape, f), f) == shape
        assert M.flagged(M.flagged(shape, M.SWAP), M.REVERSE) == M.flagged(shape, M.SWAP | M.REVERSE) == M.flagged(M.flagged(shape, M.REVERSE), M.SWAP)


# ---- the text side ----
def _record(rng, k, strand=None, trimmed=True, runs=None):
    """a record as a PAF line has it, over sequences long enough to hold it"""
    if runs is not None:
        trimmed = False
    else:
        runs = _random_runs(rng)
    if trimmed:  # what the align phase writes: aligned at both ends
        runs = [(3, "=")] + [r for r in runs] + [(2, "X" if runs[-1][1] == "=" else "=")]
        runs = [r for i, r in enumerate(runs) if i == 0 or r[1] != runs[i - 1][1]]
    _, plen, tlen = LM.columns(runs)
    qsize, tsize = tlen + rng.randrange(0, 500), plen + rng.randrange(0, 500)
    qs, ts = rng.randrange(0, qsize - tlen + 1), rng.randrange(0, tsize - plen + 1)
    return dict(qname="q#%d#chr%d" % (k % 3, k), qsize=qsize, qs=qs, qe=qs + tlen, strand=strand or rng.choice("+-"), tname="t#1#chr%d" % (k % 2), tsize=tsize,
                ts=ts, te=ts + plen, runs=runs)


def _spec(records, swap):
    """the hook's input: every record with what the device says of its problem (the model's, under the flags the issue of the file asks for)"""
    out, flags = [], []
    for r in records:
        f = (M.SWAP | (M.REVERSE if r["strand"] == "-" else 0)) if swap else 0
        flags.append(f)
        blocks, per = M.chain_problems([(r["runs"], f)])
        out.append("R\t%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % ((r["qname"], r["qsize"], r["qs"], r["qe"], r["strand"], r["tname"], r["tsize"], r["ts"],
                                                                          r["te"], per[0][8]) + per[0][4:8]))
        out += ["B\t%d\t%d\t%d" % b[:3] for b in blocks]
    return "\n".join(out) + "\n", flags


@pytest.mark.parametrize("swap", [False, True], ids=["plain", "swapped"])
@pytest.mark.parametrize("trimmed", [True, False], ids=["trimmed", "gaps_at_the_ends"])
def test_hook_byte_for_byte(swap, trimmed):
    rng = random.Random(0x7E57 + swap + 2 * trimmed)
    records = [_record(rng, k, trimmed=trimmed) for k in range(60)]
    records.insert(7, _record(rng, 99, runs=P("2I3D")))  # no block: no chain, and no id is spent on it
    records.insert(9, _record(rng, 98, "-", runs=P("17=")))  # a one-block chain on -
    assert {r["strand"] for r in records} == {"+", "-"}
    spec, flags = _spec(records, swap)
    got, got_flags = capi.host_chain_lines(spec, swap)
    want = M.chain_text(records, swap)
    assert got == want and got_flags == flags
    chains = M.parse_chains(got)
    n_chains = sum(1 for r in records if any(op in "=X" for _, op in r["runs"]))
    assert n_chains <= len(records) - 1 and [c[0]["id"] for c in chains] == list(range(1, n_chains + 1)) and any(len(c[1]) == 1 for c in chains)
    for head, blocks in chains:  # what every chain must add up to
        assert head["tstrand"] == "+" and blocks[-1][1:] == (0, 0)
        assert sum(b[0] + b[1] for b in blocks) == head["tend"] - head["tstart"] and sum(b[0] + b[2] for b in blocks) == head["qend"] - head["qstart"]
        assert 0 <= head["tstart"] < head["tend"] <= head["tsize"] and 0 <= head["qstart"] < head["qend"] <= head["qsize"]


def test_hook_spelled_out():
    """numbers written by hand: the - coordinate flip at qSize, a one-block chain, the swapped file of a - record"""
    r = dict(qname="q", qsize=1000, qs=100, qe=112, strand="-", tname="t", tsize=2000, ts=500, te=513, runs=P("4=3D2I6="))
    one_block = dict(qname="q", qsize=50, qs=0, qe=50, strand="-", tname="t", tsize=60, ts=10, te=60, runs=P("20=5X25="))
    spec, _ = _spec([r, one_block], False)
    assert capi.host_chain_lines(spec, False)[0] == (b"chain 10 t 2000 + 500 513 q 1000 - 888 900 1\n4\t3\t2\n6\n\n"
                                                     b"chain 45 t 60 + 10 60 q 50 - 0 50 2\n50\n\n")
    spec, flags = _spec([r, one_block], True)
    assert flags == [3, 3] and capi.host_chain_lines(spec, True) == (b"chain 10 q 1000 + 100 112 t 2000 - 1487 1500 1\n6\t2\t3\n4\n\n"
                                                                     b"chain 45 q 50 + 0 50 t 60 - 0 50 2\n50\n\n", [3, 3])
    assert capi.host_chain_lines("", False) == (b"", [])
    for bad in ("X\t1\n", "B\t1\t2\t3\n", "R\tq\t10\n", "R\tq\t10\t0\t5\t+\tt\t10\t0\t5\t5\t0\t0\t0\t0\nB\t5\t0\n"):
        with pytest.raises(capi.WfmError):
            capi.host_chain_lines(bad, False)


# ---- a ten-line liftOver through the files ----
CIGARS = ["10=", "4=3D4=", "4=2I3D4=", "3=2X4=1I2=", "2I5=2D", "1D1I3=1X1D1D2=2I7=3D"]


@pytest.mark.parametrize("strand", ["+", "-"])
def test_lift_pos_of_every_aligned_column(strand):
    for k, cigar in enumerate(CIGARS):
        runs = P(cigar)
        cols, plen, tlen = LM.columns(runs)
        r = dict(qname="q", qsize=tlen + 30, qs=7 + k, qe=7 + k + tlen, strand=strand, tname="t", tsize=plen + 40, ts=11, te=11 + plen, runs=runs)
        text = M.chain_text([r])
        swapped = M.chain_text([r], swap=True)
        aligned = 0
        for p, t, op in cols:
            fwd = r["qs"] + t if strand == "+" else r["qe"] - 1 - t  # the text is the query window as aligned: reverse-complemented on -
            if op in "=X":
                aligned += 1
                assert M.lift_pos(text, "t", r["ts"] + p) == [("q", strand, fwd)]
                assert M.lift_pos(swapped, "q", fwd) == [("t", strand, r["ts"] + p)]  # the inverse map
            elif op == "D":
                assert M.lift_pos(text, "t", r["ts"] + p) == []
            else:
                assert M.lift_pos(swapped, "q", fwd) == []
        assert aligned and M.lift_pos(text, "t", r["ts"] - 1) == [] and M.lift_pos(text, "t", r["te"]) == [] and M.lift_pos(text, "x", r["ts"]) == []


# ---- the command line ----
def _cli(args):
    return subprocess.run(["timeout", "-k", "10", "60", CLI] + args, capture_output=True, text=True)


@pytest.mark.parametrize("args, message", [
    (["--chain-swap"], "--chain-swap needs --chain FILE"),
    (["--chain-paf", "x.paf"], "--chain-paf needs --chain FILE"),
    (["--chain-paf", "x.paf", "--chain-swap"], "--chain-swap needs --chain FILE"),
    (["--chain", "x.chain", "-m"], "--chain writes chains of alignments: it cannot be combined with -m"),
    (["--chain", "x.chain", "--chain-swap", "--verify-paf", "x.paf"], "--chain belongs to the align phase: it cannot be combined with --verify-paf"),
    (["--chain", "x.chain", "--chain-paf", "x.paf", "--left-align"], "--chain-paf runs nothing else"),
    (["--chain", "x.chain", "--lift-paf", "x.paf", "--lift", "x.bed", "--lift-out", "x.tsv"], "--lift-paf runs nothing else"),
    (["--chain"], "missing value for --chain"),
])
def test_cli_refused_combinations(args, message):
    r = _cli(args + ["t.fa"] if args != ["--chain"] else args)
    assert r.returncode == 1 and message in r.stderr, (r.returncode, r.stderr)


def test_cli_help_names_the_switches():
    r = _cli(["--help"])
    assert all(s in r.stdout + r.stderr for s in ("--chain FILE", "--chain-swap", "--chain-paf FILE"))
