"""GPU tests of --lift: wfm_liftset_* and wfm_lift_runs word for word against the brute-force model (tests/lift_model.py) on hand cases,
nested intervals, adversarial gap chains, the 256-run rounds, the candidate windows, refused problems and calls, positions beyond 2^32,
chunked output and a seeded fuzz; then the align driver on the synthetic pangenome of tests/test_left_align_gpu.py and the command line."""
import os
import random
import re
import subprocess
import types

import pytest

from tests import lift_model as M
from tests import test_left_align_gpu as LT  # its synthetic pangenome (nothing of it is collected from here)
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
SPANS = capi.WFM_LIFT_SPANS
P = M.parse


# ---- 1. the C ABI against the model ----
def _layout(problems, junk=0, reverse=False):
    """the run buffer and [(base, runs_off, n_runs)]: `junk` words of rubbish before, between and behind the problems' runs; reverse: the
    problems' runs lie in the buffer in the opposite order, so runs_off descends"""
    rubbish = [0xFFFFFFFF, 0, 7, (5 << 2) | 3]
    buf, where = [], [None] * len(problems)
    order = range(len(problems) - 1, -1, -1) if reverse else range(len(problems))
    for k in order:
        buf += [rubbish[(k + j) % 4] for j in range(junk)]
        where[k] = (problems[k][0], len(buf), len(problems[k][1]))
        buf += M.words(problems[k][1])
    buf += rubbish[:junk]
    return buf, where


def _lift(gpu, problems, intervals, n_bases, junk=0, reverse=False):
    """(lifts, per) of one call on a fresh liftset, as lists of tuples like the model's"""
    s = gpu.liftset(intervals, n_bases)
    try:
        buf, where = _layout(problems, junk, reverse)
        lifts, per = s.lift(where, buf)
        return lifts.tolist(), per.tolist(), lifts.tobytes()
    finally:
        s.close()


def _assert_model(gpu, problems, intervals, n_bases, **kw):
    lifts, per, _ = _lift(gpu, problems, intervals, n_bases, **kw)
    want_lifts, want_per = M.lift_problems(problems, intervals, n_bases)
    assert per == want_per
    assert lifts == want_lifts
    return lifts, per


# name, n_bases, problems [(base, runs)], intervals (sorted before use)
HAND = [
    ("interval_equal_to_the_span", 100, [(10, P("20="))], [(10, 30)]),
    ("strictly_inside_one_eq_run", 100, [(10, P("20="))], [(13, 17)]),
    ("start_in_a_D_run", 100, [(0, P("4=3D4="))], [(5, 9)]),
    ("end_in_a_D_run", 100, [(0, P("4=3D4="))], [(2, 6)]),
    ("wholly_inside_a_D_run", 100, [(0, P("4=3D4="))], [(4, 7), (5, 6)]),
    ("over_3D2I_alone", 100, [(0, P("4=3D2I4="))], [(4, 7)]),
    ("over_2I3D_alone", 100, [(0, P("4=2I3D4="))], [(4, 7)]),
    ("I_directly_before_p0", 100, [(0, P("4=2I4="))], [(4, 8)]),
    ("I_directly_after_p1", 100, [(0, P("4=2I4="))], [(0, 4)]),
    ("I_strictly_inside", 100, [(0, P("4=2I4="))], [(2, 6)]),
    ("first_run_I", 100, [(0, P("2I5="))], [(0, 5), (0, 1)]),
    ("last_run_I", 100, [(0, P("5=2I"))], [(0, 5), (4, 5)]),
    ("first_run_D", 100, [(0, P("2D5="))], [(0, 1), (0, 2), (0, 7), (1, 3)]),
    ("last_run_D", 100, [(0, P("5=2D"))], [(0, 7), (4, 6), (5, 7), (6, 7)]),
    ("clipped_on_the_left", 200, [(100, P("10="))], [(90, 105)]),
    ("clipped_on_the_right", 200, [(100, P("10="))], [(105, 200)]),
    ("clipped_on_both_sides", 200, [(100, P("3=1X2D1I4="))], [(0, 200)]),
    ("end_equal_to_a_is_excluded", 200, [(100, P("10="))], [(90, 100), (99, 101)]),
    ("start_equal_to_b_is_excluded", 200, [(100, P("10="))], [(109, 111), (110, 120)]),
    ("X_runs_counted_in_x", 100, [(0, P("3=2X4=1X"))], [(0, 10), (2, 6), (3, 5), (9, 10)]),
    ("only_gaps", 100, [(3, P("2I3D1I"))], [(0, 100), (4, 5)]),
    ("one_base", 100, [(99, P("1X"))], [(0, 100), (99, 100)]),
]


@pytest.mark.parametrize("name,n_bases,problems,intervals", HAND, ids=[h[0] for h in HAND])
def test_hand_cases_word_for_word(gpu, name, n_bases, problems, intervals):
    lifts, per = _assert_model(gpu, problems, sorted(intervals), n_bases)
    assert per[0][0] == 0


def test_hand_cases_spelled_out(gpu):
    """a few of the above against numbers written by hand, not the model's"""
    got = lambda c, a, b: [l[2:] for l in _lift(gpu, [(0, P(c))], [(a, b)], 100)[0]]
    assert got("4=3D4=", 5, 9) == [(7, 9, 4, 6, 2, 0)]
    assert got("4=3D4=", 4, 7) == [(4, 4, 4, 4, 0, 0)]
    assert got("4=2I3D4=", 4, 7) == [(4, 4, 6, 6, 0, 0)]
    assert got("4=2I4=", 2, 6) == [(2, 6, 2, 8, 4, 0)] and got("4=2I4=", 4, 8) == [(4, 8, 6, 10, 4, 0)] and got("4=2I4=", 0, 4) == [(0, 4, 0, 4, 4, 0)]
    assert got("5=2I", 4, 5) == [(4, 5, 4, 5, 1, 0)] and got("5=2D", 5, 7) == [(5, 5, 5, 5, 0, 0)]
    assert got("3=2X4=", 2, 6) == [(2, 6, 2, 6, 2, 2)]


def test_nested_intervals_need_the_running_maximum(gpu):
    """one interval over everything, listed first, and 300 short ones behind it: most problems overlap only the long one, which a
    window taken from `start` alone would miss"""
    n_bases = 40000
    intervals = [(0, n_bases)] + [(100 + 20 * i, 110 + 20 * i) for i in range(300)]
    problems = [(50, P("30=")), (104, P("3=2D1I4=")), (7000, P("100=5D100=")), (20000, P("7X")), (39990, P("10=")), (6085, P("25=")), (0, P("120="))]
    lifts, per = _assert_model(gpu, problems, intervals, n_bases)
    assert [p[3] for p in per] == [1, 2, 1, 1, 1, 2, 2]
    assert all(any(l[0] == k and l[1] == 0 for l in lifts) for k in range(len(problems)))


def test_adversarial_gap_chain(gpu):
    """10 000 alternating 1I1D between two 5= runs: every endpoint inside the chain has 10^4 gap runs to its nearest aligned base"""
    runs = P("5=") + P("1I1D") * 10000 + P("5=")
    n_bases = 20000
    intervals = sorted([(1000, 9000), (3, 5000), (5000, 10008), (2000, 2001), (4, 6), (5, 10005), (10004, 10006), (0, 10010), (9999, 10005)] +
                       [(5 + 199 * i, 5 + 199 * i + 1 + 13 * i) for i in range(40)])
    lifts, per = _assert_model(gpu, [(7, runs)], [(a + 7, b + 7) for a, b in intervals], n_bases)
    assert per[0][3] == len(intervals) and sum(1 for l in lifts if l[6] + l[7] == 0) >= 40


def _mixed(n_runs, seed):
    """n_runs runs of all four ops, never two of a kind in a row, aligned at both ends"""
    rng = random.Random(seed)
    runs, last = [], None
    for k in range(n_runs):
        op = rng.choice([o for o in "=XID" if o != last]) if 0 < k < n_runs - 1 else "="
        if op == last:
            op = "X"
        runs.append((rng.randrange(1, 4), op))
        last = op
    return runs


@pytest.mark.parametrize("n_runs", [1, 255, 256, 257, 1025])
def test_run_counts_on_the_round_carry(gpu, n_runs):
    runs = _mixed(n_runs, n_runs)
    _, plen, _ = M.columns(runs)
    # where the 256th, 512th, ... run begins in the pattern: intervals that straddle, begin at and end at those places
    edges, p = [], 0
    for k, (n, op) in enumerate(runs):
        if k and k % 256 == 0:
            edges.append(p)
        if op != "I":
            p += n
    intervals = {(0, plen), (0, 1), (plen - 1, plen)}
    for e in edges:
        for a, b in ((e - 3, e + 3), (e, e + 1), (e - 1, e), (e - 2, plen), (0, e), (0, e + 1)):
            if 0 <= a < b <= plen:
                intervals.add((a, b))
    base = 11
    _assert_model(gpu, [(base, runs)], sorted((a + base, b + base) for a, b in intervals), plen + 40)


@pytest.mark.parametrize("window", [0, 1, 256, 257])
def test_candidate_windows(gpu, window):
    """`window` intervals overlap the one problem; others lie before and behind it"""
    runs = _mixed(90, 5)
    _, plen, _ = M.columns(runs)
    base = 1000
    inside = [(base - 5 + (i * (plen + 4)) // max(window, 1), base - 5 + (i * (plen + 4)) // max(window, 1) + 7 + i % 5) for i in range(window)]
    inside = [(a, b) for a, b in inside if a < base + plen and b > base]
    outside = [(10, 20), (900, 1000), (base + plen, base + plen + 9), (5000, 5001)]
    lifts, per = _assert_model(gpu, [(base, runs)], sorted(inside + outside), 6000)
    assert per[0][3] == len(inside) and (window < 256 or len(inside) >= window - 8)


def test_junk_between_the_runs_and_descending_offsets(gpu):
    problems = [(10 + 300 * k, _mixed(20 + 37 * k, k)) for k in range(9)]
    intervals = sorted((a, a + w) for a in range(0, 3000, 41) for w in (3, 90))
    a, _ = _assert_model(gpu, problems, intervals, 8000, junk=5)
    b, _ = _assert_model(gpu, problems, intervals, 8000, junk=3, reverse=True)
    assert a == b


def test_refused_problems_leave_their_neighbours_alone(gpu):
    intervals = [(0, 100), (5, 8), (40, 60), (95, 100)]
    good = [(2, P("10=")), (30, P("4=2D1I9=")), (90, P("10="))]
    bad = [(0, P("3=0D2=")), (95, P("10=")), (101, P("1=")), (25, [])]
    problems = [good[0], bad[0], bad[1], good[1], bad[2], bad[3], good[2]]
    lifts, per = _assert_model(gpu, problems, intervals, 100)
    assert [p[0] for p in per] == [0, SPANS, SPANS, 0, SPANS, SPANS, 0] and all(p[3] == 0 for p in per if p[0])
    alone, _, _ = _lift(gpu, good, intervals, 100)
    assert [l[1:] for l in lifts] == [l[1:] for l in alone]  # (the problem numbers differ, nothing else)


def test_a_run_range_past_the_buffer(gpu):
    s = gpu.liftset([(0, 50)], 100)
    try:
        words = M.words(P("10="))
        for where in ([(0, 0, 2)], [(0, 1, 1)], [(0, 0, 1), (0, 5, 1)]):
            with pytest.raises(capi.WfmError, match="leave the run buffer"):
                s.lift(where, words)
        lifts, per = s.lift([(5, 0, 1)], words)  # the handle and the set are usable afterwards
        assert lifts.tolist() == [(0, 0, 0, 10, 0, 10, 10, 0)] and per.tolist() == [(0, 1, 0, 1)]
    finally:
        s.close()


@pytest.mark.parametrize("intervals,n_bases", [
    ([(5, 9), (4, 6)], 100), ([(5, 9), (5, 8)], 100), ([(5, 5)], 100), ([(7, 5)], 100), ([(90, 101)], 100), ([(0, 1)], 0)])
def test_create_refuses(gpu, intervals, n_bases):
    with pytest.raises(capi.WfmError, match="wfm_liftset_create"):
        gpu.liftset(intervals, n_bases)
    assert _lift(gpu, [(0, P("3="))], [(0, 3)], 10)[0] == [(0, 0, 0, 3, 0, 3, 3, 0)]  # the handle is usable afterwards


def test_no_intervals_and_no_problems(gpu):
    lifts, per, _ = _lift(gpu, [(0, P("10=")), (95, P("10="))], [], 100)
    assert lifts == [] and per == [(0, 1, 0, 0), (SPANS, 1, 0, 0)]
    lifts, per, _ = _lift(gpu, [], [(0, 10), (0, 10)], 100)
    assert lifts == [] and per == []
    lifts, per, _ = _lift(gpu, [(50, P("10="))], [(0, 10), (60, 70)], 100)  # problems, intervals, no pairs
    assert lifts == [] and per == [(0, 1, 0, 0)]


def test_positions_beyond_32_bits(gpu):
    n_bases = (1 << 33) + 12345
    g = (1 << 32) + 999
    problems = [(g, P("50=3D2I40=")), (5, P("20=")), (n_bases - 30, P("30=")), (n_bases - 29, P("30="))]
    intervals = sorted([(0, n_bases), (g - 10, g + 10), (g + 49, g + 54), (g + 92, n_bases), (1 << 32, (1 << 32) + 5), (n_bases - 1, n_bases), (3, 9)])
    lifts, per = _assert_model(gpu, problems, intervals, n_bases)
    assert [p[0] for p in per] == [0, 0, 0, SPANS] and per[0][3] == 4


def _many(seed=0xBEEF, n_prob=60):
    rng = random.Random(seed)
    problems = [(rng.randrange(0, 5000), _mixed(rng.randrange(1, 60), seed + k)) for k in range(n_prob)]
    intervals = sorted((a, a + rng.randrange(1, 400)) for a in (rng.randrange(0, 5500) for _ in range(150)))
    return problems, intervals, 6000


def test_chunked_output_is_the_same_bytes(gpu, monkeypatch):
    problems, intervals, n_bases = _many()
    lifts, per, raw = _lift(gpu, problems, intervals, n_bases)
    assert len(lifts) > 200 and max(p[3] for p in per) > 3
    monkeypatch.setenv("WFM_LIFT_OUT_MB", "0.0001")  # three lifts: nearly every problem a chunk of its own, many of them larger than that
    lifts2, per2, raw2 = _lift(gpu, problems, intervals, n_bases)
    assert raw2 == raw and per2 == per
    monkeypatch.setenv("WFM_LIFT_OUT_MB", "0.002")
    assert _lift(gpu, problems, intervals, n_bases)[2] == raw


def test_two_calls_give_the_same_bytes(gpu):
    problems, intervals, n_bases = _many(seed=0xFACE)
    s = gpu.liftset(intervals, n_bases)
    try:
        buf, where = _layout(problems)
        a, pa = s.lift(where, buf)
        b, pb = s.lift(where, buf)
        assert a.tobytes() == b.tobytes() and pa.tobytes() == pb.tobytes() and len(a)
    finally:
        s.close()


def test_more_intervals_than_one_scan_block(gpu):
    """the running maximum across blocks of WFM_LIFT_SCAN_BLOCK intervals: a long interval early in block 0 is the only one that reaches
    problems whose other candidates lie two blocks further on"""
    n = 2 * capi.WFM_LIFT_SCAN_BLOCK + 77
    intervals = [(0, 3), (1, 9000)] + [(10 + 4 * i, 13 + 4 * i) for i in range(n)]
    n_bases = 10000
    problems = [(8990, P("5=")), (8400, P("3=1D3=")), (4 * capi.WFM_LIFT_SCAN_BLOCK + 9, P("9=")), (9000, P("4=")), (0, P("2="))]
    lifts, per = _assert_model(gpu, problems, intervals, n_bases)
    assert [p[3] for p in per] == [1, 4, 3, 0, 2]


def _random_runs(rng):
    n = rng.randrange(1, 40)
    runs, last = [], None
    for _ in range(n):
        op = rng.choice([o for o in "=XID" if o != last])  # gaps at the ends too
        runs.append((rng.randrange(1, 9), op))
        last = op
    return runs


def test_fuzz_equals_the_model(gpu):
    rng = random.Random(0x11F7)
    n_bases = 30000
    problems = []
    for _ in range(200):
        runs = _random_runs(rng)
        problems.append((rng.randrange(0, n_bases - 400), runs))
    intervals = [(0, n_bases), (100, 25000)]
    for _ in range(498):
        a = rng.randrange(0, n_bases - 1)
        intervals.append((a, min(n_bases, a + rng.choice([1, 2, 5, 30, 300, 4000]))))
    intervals.sort()
    lifts, per = _assert_model(gpu, problems, intervals, n_bases, junk=2)
    assert len(lifts) > 1000 and any(l[6] + l[7] == 0 for l in lifts)


# ---- 2. the align driver ----
def _align(handles, case, out, bed, lifted, left=False, **params):
    capi.set_lift(bed, lifted)
    capi.set_left_align(left)
    try:
        if len(handles) == 1:
            capi.align_paf(handles[0], case.fa, case.paf, out, params=params or None)
        else:
            capi.align_paf_multi(handles, case.fa, case.paf, out, params=params or None)
        return open(out, "rb").read(), (open(lifted).read() if lifted else None), capi.lift_counts()
    finally:
        capi.set_lift(None, None)
        capi.set_left_align(False)


def _bed_of(names, lengths):
    """1 kb windows tiling every sequence, a few nested genes, one interval over a whole sequence, and lines to skip"""
    out = ["# genes", "track name=x"]
    for name, n in zip(names, lengths):
        out += ["%s\t%d\t%d\tw%d" % (name, a, min(n, a + 1000), a // 1000) for a in range(0, n, 1000)]
        out += ["%s\t0\t%d" % (name, n), "%s\t1990\t2060\trepeat\t0\t-" % name, "%s\t2000\t2004\ttiny" % name, "%s\t%d\t%d\tbeyond" % (name, n - 1, n + 1)]
    out += ["nobody#1#chrZ\t0\t10\tunknown", ""]
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows, a BED over it, the aligned PAF of a run without the switch and the lift file of one with it: made
    once, never changed"""
    d = str(tmp_path_factory.mktemp("lift"))
    fa, paf, seqs = LT._make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, seqs=seqs, names=list(seqs), lengths=[len(s) for s in seqs.values()])
    c.bed_text = _bed_of(c.names, c.lengths)
    c.bed = os.path.join(d, "genes.bed")
    with open(c.bed, "w") as f:
        f.write(c.bed_text)
    c.text, none, counts = _align([gpu], c, os.path.join(d, "plain.paf"), None, None)
    assert none is None and counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20
    c.with_text, c.lifted, c.counts = _align([gpu], c, os.path.join(d, "with.paf"), c.bed, os.path.join(d, "with.lift"))
    return c


def test_driver_plain(gpu, case):
    assert case.with_text == case.text
    want, counts = M.lift_paf(case.lines, case.bed_text, case.names, case.lengths)
    assert case.lifted == want and case.counts == counts
    strands = {l.split("\t")[4] for l in want.splitlines()}
    # (every record overlaps the interval over its whole sequence and a 1 kb window at least)
    assert strands == {"+", "-"} and counts[1] >= 2 * len(case.lines) and counts[3] == 4 + len(case.names)
    for l in want.splitlines():  # the shape of a line: 14 columns, integers but for the names and the strand
        f = l.split("\t")
        assert len(f) == 14 and all(v.isdigit() for k, v in enumerate(f) if k not in (0, 3, 4, 5))
    # the switch off again: the bytes of the run without it, no counts
    again, none, counts = _align([gpu], case, os.path.join(case.dir, "off.paf"), None, None)
    assert again == case.text and none is None and counts == (0, 0, 0, 0)


def test_driver_with_left_align(gpu, case):
    plain, _, _ = _align([gpu], case, os.path.join(case.dir, "la0.paf"), None, None, left=True)
    text, lifted, counts = _align([gpu], case, os.path.join(case.dir, "la.paf"), case.bed, os.path.join(case.dir, "la.lift"), left=True)
    assert text == plain != case.text
    want, want_counts = M.lift_paf(text.decode().splitlines(), case.bed_text, case.names, case.lengths)
    assert lifted == want and counts == want_counts
    assert lifted != case.lifted  # the normalised runs are lifted: a gap that moved moves an endpoint


def test_driver_two_handles_on_one_device(gpu, case):
    h2 = capi.Handle(0)
    try:
        text, lifted, counts = _align([gpu, h2], case, os.path.join(case.dir, "m.paf"), case.bed, os.path.join(case.dir, "m.lift"))
    finally:
        h2.close()
    assert text == case.text and lifted == case.lifted and counts == case.counts


def test_driver_filtered_records_have_no_lines(gpu, case):
    text, lifted, counts = _align([gpu], case, os.path.join(case.dir, "f.paf"), case.bed, os.path.join(case.dir, "f.lift"), min_alignment_length=5000)
    lines = text.decode().splitlines()
    assert 0 < len(lines) < len(case.lines)
    want, want_counts = M.lift_paf(lines, case.bed_text, case.names, case.lengths)
    assert lifted == want and counts == want_counts


def test_driver_two_gpus(gpu, case):
    if capi.load().wfm_device_count() < 2:
        pytest.skip("one GPU on this node: the two-GPU file cannot be made")
    h2 = capi.Handle(1)
    try:
        text, lifted, counts = _align([gpu, h2], case, os.path.join(case.dir, "g2.paf"), case.bed, os.path.join(case.dir, "g2.lift"))
    finally:
        h2.close()
    assert text == case.text and lifted == case.lifted and counts == case.counts


def test_lift_paf_entry_point(gpu, case):
    out = os.path.join(case.dir, "offline.lift")
    counts = capi.lift_paf(gpu, case.fa, os.path.join(case.dir, "plain.paf"), case.bed, out)
    assert open(out).read() == case.lifted and counts == case.counts


# ---- 3. the command line ----
def _cli(args, cwd=None):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "120", CLI] + args, capture_output=True, text=True, cwd=cwd)


COUNTS = r"\[wfmash::lift\] (\d+) records lifted, (\d+) lines written, (\d+) of them empty, (\d+) BED lines skipped"


def test_cli_beside_the_other_switches_and_from_the_paf(case):
    out, lifted, bg = os.path.join(case.dir, "cli.paf"), os.path.join(case.dir, "cli.lift"), os.path.join(case.dir, "cli.bg")
    r = _cli(["--lift", case.bed, "--lift-out", lifted, "--coverage", bg, "--cs", "--verify", "-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    lines = open(out).read().splitlines()
    assert [l.rpartition("\tcs:Z:")[0] for l in lines] == case.lines
    assert open(lifted).read() == case.lifted
    m = re.search(COUNTS, r.stderr)
    assert m and tuple(int(x) for x in m.groups()) == case.counts
    # without the switch: the plain run's bytes
    out0 = os.path.join(case.dir, "cli0.paf")
    r = _cli(["-i", case.paf, "--out", out0, case.fa])
    assert r.returncode == 0 and open(out0, "rb").read() == case.text
    # the file again from the PAF the run wrote, byte for byte
    lifted2 = os.path.join(case.dir, "cli2.lift")
    r = _cli(["--lift-paf", out, "--lift", case.bed, "--lift-out", lifted2, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert open(lifted2).read() == case.lifted
    assert "%d lines lifted, 0 skipped" % len(lines) in r.stderr and "%d lifts written, %d of them empty" % case.counts[1:3] in r.stderr


@pytest.mark.parametrize("args, message", [
    (["--lift", "x.bed"], "--lift needs --lift-out FILE"),
    (["--lift-out", "x.tsv"], "--lift-out needs --lift IN.bed"),
    (["--lift-paf", "x.paf"], "--lift-paf needs --lift IN.bed and --lift-out FILE"),
    (["--lift", "x.bed", "--lift-out", "x.tsv", "-m"], "--lift lifts through alignments: it cannot be combined with -m"),
    (["--lift", "x.bed", "--lift-out", "x.tsv", "--verify-paf", "x.paf"], "--lift belongs to the align phase: it cannot be combined with --verify-paf"),
    (["--lift", "x.bed", "--lift-out", "x.tsv", "--lift-paf", "x.paf", "--left-align"], "--lift-paf runs nothing else"),
])
def test_cli_refused_combinations(args, message):
    r = _cli(args + ["t.fa"])
    assert r.returncode == 1 and message in r.stderr, (r.returncode, r.stderr)
