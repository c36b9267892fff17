"""The transitive closure as far as it can be checked without a device: tests/trans_model.py against tests/lift_model.py and against
itself (the properties the closure has by definition), its fast NumPy form against the brute force, and the surface of the library."""
import ctypes as C
import os
import random
import re

import pytest

from tests import lift_model as LM
from tests import trans_model as TM
from wfmash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_runs(rng, n_runs, max_len=4):
    """runs whose neighbours differ in op, with one aligned run at least"""
    while True:
        runs, last = [], None
        for _ in range(n_runs):
            op = rng.choice([o for o in "=XID" if o != last])
            runs.append((rng.randint(1, max_len), op))
            last = op
        if any(op in "=X" for _, op in runs):
            return runs


def random_world(rng, n_bases=200, max_records=6):
    records = []
    for _ in range(rng.randint(1, max_records)):
        while True:
            runs = random_runs(rng, rng.randint(1, 9))
            P, T = TM.spans(runs)
            if P <= n_bases and T <= n_bases:
                break
        records.append((rng.randint(0, n_bases - P), rng.randint(0, n_bases - T), rng.random() < 0.4, runs))
    return records


def swapped(rec):
    """the record seen from its query: target and query change places, I and D with them; the columns run backwards where it is reversed"""
    t, q, rev, runs = rec
    sw = [(n, {"I": "D", "D": "I"}.get(op, op)) for n, op in runs]
    return (q, t, rev, sw[::-1] if rev else sw)


def test_forward_hull_is_the_lift_moved_to_the_world():
    rng = random.Random(0x7a)
    for _ in range(300):
        runs = random_runs(rng, rng.randint(1, 12))
        P, T = TM.spans(runs)
        t, q, rev = rng.randint(0, 50), rng.randint(0, 50), rng.random() < 0.5
        cols, _, _ = LM.columns(runs)
        at = LM.by_base(cols)
        for _ in range(10):
            a = rng.randint(0, t + P + 3)
            b = rng.randint(a + 1, t + P + 6)
            lo, hi = max(a, t), min(b, t + P)
            got = TM.hull((t, q, rev, runs), False, a, b)
            if lo >= hi:
                assert got is None
                continue
            p0, p1, t0, t1, eq, x = LM.lift_columns(at, lo - t, hi - t)
            if eq + x == 0:
                assert got is None
            else:
                assert got == ((q + T - t1, q + T - t0) if rev else (q + t0, q + t1))


def test_back_hull_is_the_forward_hull_of_the_swapped_record():
    rng = random.Random(0x7b)
    for _ in range(300):
        rec = (rng.randint(0, 40), rng.randint(0, 40), rng.random() < 0.5, random_runs(rng, rng.randint(1, 12)))
        sw = swapped(rec)
        assert sorted(TM.aligned_pairs(sw)) == sorted((b, a) for a, b in TM.aligned_pairs(rec))
        for _ in range(10):
            a = rng.randint(0, 80)
            b = rng.randint(a + 1, 90)
            assert TM.hull(rec, True, a, b) == TM.hull(sw, False, a, b)
            assert TM.hull(rec, False, a, b) == TM.hull(sw, True, a, b)


def covered(R):
    return {x for a, b in R for x in range(a, b)}


def test_closure_properties_on_small_worlds():
    rng = random.Random(0x7c)
    for _ in range(60):
        records = random_world(rng)
        a = rng.randint(0, 190)
        seed = (a, rng.randint(a + 1, min(200, a + 12)))
        levels = [TM.closure(records, seed, d)[0] for d in range(1, 9)]
        for lo, hi in zip([[seed]] + levels, levels):
            assert covered(lo) <= covered(hi)
        shuffled = records[:]
        rng.shuffle(shuffled)
        assert [TM.closure(shuffled, seed, d)[0] for d in range(1, 9)] == levels
        fixed, rounds = TM.closure(records, seed, 0)
        first = next((k for k in range(len(levels)) if levels[k] == ([[seed]] + levels)[k]), None)
        if first is not None:
            assert fixed == levels[first] and rounds == first + 1
        else:
            assert rounds > len(levels)
        assert TM.closure(records, seed, 0)[0] == TM.closure(records, seed, 50)[0] or rounds > 50
        for d in (0, 1, 2, 3, 5):
            assert TM.closure(records, seed, d, skip=True)[0] == TM.closure(records, seed, d, skip=False)[0]


def test_fast_form_equals_the_brute_force():
    rng = random.Random(0x7d)
    for _ in range(300):
        records = random_world(rng)
        fast = TM.Fast(records)
        for k, rec in enumerate(records):
            for back in (False, True):
                for _ in range(4):
                    a = rng.randint(0, 199)
                    b = rng.randint(a + 1, 200)
                    assert fast.hull(2 * k + back, a, b) == TM.hull(rec, back, a, b)
        seeds = []
        for _ in range(3):
            a = rng.randint(0, 190)
            seeds.append((a, rng.randint(a + 1, min(200, a + 15))))
        for depth in (0, 1, 2):
            assert fast.closures(seeds, depth) == TM.closures(records, seeds, depth)


def test_two_pieces_that_meet_inside_a_gap_keep_the_insertion():
    # a record 4= 3I 4=: the halves of the target side lift to query pieces three bases apart; merged first, the seed spans the gap
    rec = (0, 100, False, LM.parse("4=3I4="))
    assert TM.closure([rec], (0, 8), 1)[0] == [(0, 8), (100, 111)]
    assert TM.merge([TM.hull(rec, False, 0, 4), TM.hull(rec, False, 4, 8)]) == [(100, 104), (107, 111)]


def test_library_surface():
    L = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfmash_hip.h")).read(), flags=re.S)
    names = ["wfm_trans_create", "wfm_trans_free", "wfm_trans_add", "wfm_trans_closure", "wfm_trans_export", "wfm_trans_import",
             "wfm_trans_counts", "wfm_trans_free_list"]
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", text) and name in capi.EXPORTS and hasattr(L, name), name
    for name, value in (("WFM_TRANS_REVERSE", capi.WFM_TRANS_REVERSE), ("WFM_TRANS_SPANS", capi.WFM_TRANS_SPANS),
                        ("WFM_TRANS_SCAN_BLOCK", capi.WFM_TRANS_SCAN_BLOCK)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", text)
        assert m and int(m.group(1)) == value, name
    assert TM.REVERSE == capi.WFM_TRANS_REVERSE and TM.SPANS == capi.WFM_TRANS_SPANS
    assert capi.TRANS_PROB_DTYPE.itemsize == 32 and capi.TRANS_REC_DTYPE.itemsize == 32 and capi.TRANS_WORD_DTYPE.itemsize == 16
    assert capi.TRANS_IV_DTYPE.itemsize == 24 and capi.TRANS_SEED_DTYPE.itemsize == 24
    assert hasattr(capi.Handle, "transitive") and hasattr(capi, "Transitive")


# ---- the text side and the command line ----
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
TNAMES, TLENGTHS = ["chrA", "chrB", "empty", "chrC"], [100, 50, 0, 70]
QNAMES, QLENGTHS = ["chrB", "hapX", "chrA", "hapY"], [50, 30, 100, 40]

BED = ("# a comment\n"
       "chrA\t10\t20\tgene1\n"
       "hapY\t0\t40\n"
       "\n"
       "track name=x\n"
       "browser position\n"
       "chrA\t5\n"
       "chrA\t5\tx\n"
       "chrQ\t1\t2\n"
       "chrB\t7\t7\n"
       "chrB\t40\t51\n"
       "hapX\t29\t30\tlast\textra\r\n"
       "chrA\t10\t20\tgene1\n"
       "chrA 1 2\n")


def test_world_and_bed_rules():
    names, lengths = TM.world(TNAMES, TLENGTHS, QNAMES, QLENGTHS)
    assert names == ["chrA", "chrB", "empty", "chrC", "hapX", "hapY"] and lengths == [100, 50, 0, 70, 30, 40]
    seeds, skipped = TM.parse_seeds(BED, names, lengths)
    assert [(s["seq"], s["start"], s["end"], s["name"]) for s in seeds] == [(0, 10, 20, "gene1"), (5, 0, 40, "."), (4, 29, 30, "last"), (0, 10, 20, "gene1")]
    assert skipped == 10
    got = capi.host_transitive_lines(TNAMES, TLENGTHS, QNAMES, QLENGTHS, BED, "")
    assert got == LM.bed_dump(seeds, skipped)


def test_lines_split_at_sequence_boundaries():
    names, lengths = TM.world(TNAMES, TLENGTHS, QNAMES, QLENGTHS)
    off = LM.offsets(lengths)
    seeds, skipped = TM.parse_seeds(BED, names, lengths)
    ivs = [(10, 20, 0), (95, 100, 0), (95, 105, 0), (100, 150, 0), (99, 151, 0), (140, 160, 0), (0, off[-1], 1), (off[4] - 1, off[4] + 1, 2),
           (off[5], off[5] + 40, 3), (149, 150, 3), (150, 151, 3)]
    spec = "".join("I\t%d\t%d\t%d\n" % (i, a, b) for a, b, i in ivs)
    want = TM.file_text(names, lengths, seeds, ivs)
    assert want.count("\n") == 1 + 1 + 2 + 1 + 3 + 2 + 5 + 2 + 1 + 1 + 1  # (the pieces of each interval, by hand)
    assert "chrA\t95\t100\tgene1\tchrA\t10\t20\nchrB\t0\t5\tgene1\tchrA\t10\t20\n" in want  # an interval over the boundary is two lines
    assert "empty" not in want
    got = capi.host_transitive_lines(TNAMES, TLENGTHS, QNAMES, QLENGTHS, BED, spec)
    assert got == LM.bed_dump(seeds, skipped) + want
    for bad in ("I\t9\t0\t1\n", "I\t0\t5\t4\n", "I\t0\t0\t%d\n" % (off[-1] + 1), "J\t0\t0\t1\n", "I\t0\t1\n"):
        with pytest.raises(capi.WfmError):
            capi.host_transitive_lines(TNAMES, TLENGTHS, QNAMES, QLENGTHS, BED, bad)


def test_strand_arithmetic_of_a_record():
    # a '-' record over the forward query window [qs, qe): its world place is the window's first base whatever the strand, and text index
    # i is base qe - 1 - i
    rec = (200, 1000 + 30, True, LM.parse("4=2D3=1I2="))
    P, T = TM.spans(rec[3])
    pairs = TM.aligned_pairs(rec)
    assert pairs[0] == (200, 1030 + T - 1) and pairs[-1] == (200 + P - 1, 1030)
    assert TM.hull(rec, False, 200, 204) == (1030 + T - 4, 1030 + T)
    assert TM.hull(rec, True, 1030, 1032) == (200 + P - 2, 200 + P)


def _cli(args):
    import subprocess
    return subprocess.run(["timeout", "-k", "10", "60", CLI] + args, capture_output=True, text=True)


def test_cli_refusals(tmp_path):
    fa = str(tmp_path / "t.fa")
    open(fa, "w").write(">a\nACGT\n")
    for args, text in ((["--transitive", "x.bed", fa], "--transitive needs --transitive-out FILE"),
                       (["--transitive-out", "x.tsv", fa], "--transitive-out needs --transitive IN.bed"),
                       (["--transitive", "x.bed", "--transitive-out", "x.tsv", "-m", fa], "cannot be combined with -m"),
                       (["--transitive", "x.bed", "--transitive-out", "x.tsv", "--verify-paf", "x.paf", fa], "cannot be combined with --verify-paf"),
                       (["--transitive", "x.bed", "--transitive-out", "x.tsv", "--transitive-depth", "-1", fa], "--transitive-depth takes a number"),
                       (["--transitive", "x.bed", "--transitive-out", "x.tsv", "--transitive-depth", "two", fa], "--transitive-depth takes a number"),
                       (["--transitive-paf", "x.paf", fa], "--transitive-paf needs --transitive IN.bed and --transitive-out FILE"),
                       (["--transitive-paf", "x.paf", "--transitive", "x.bed", "--transitive-out", "x.tsv", "--left-align", fa], "--transitive-paf runs nothing else"),
                       (["--transitive", "x.bed", "--transitive-out", "x.tsv", "--transitive-depth"], "")):
        r = _cli(args)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)
    assert "--transitive IN.bed --transitive-out FILE" in _cli(["--help"]).stderr + _cli(["--help"]).stdout


def test_host_surface():
    L = capi.load()
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfmash_host.h")).read(), flags=re.S)
    for name in ("wfmh_set_transitive", "wfmh_transitive_counts", "wfmh_transitive_paf", "wfmh_test_transitive_lines"):
        assert re.search(r"\b" + name + r"\s*\(", host) and name in capi.HOST_EXPORTS and hasattr(L, name), name
    capi.set_transitive(None, None)
    assert capi.transitive_counts() == (0, 0, 0, 0)
    assert C.sizeof(capi.AlignParams) == 88
