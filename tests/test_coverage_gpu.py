"""GPU tests of --coverage: wfm_coverage_* through capi, every result held word for word against tests/coverage_model.py; then the align
driver on the synthetic pangenome of tests/test_left_align_gpu.py and the command line."""
import os
import random
import re
import subprocess
import types

import numpy as np
import pytest

from tests import coverage_model as V
from tests import test_left_align_gpu as LT  # its synthetic pangenome (nothing of it is collected from here)
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
TILE = capi.WFM_COV_TILE
BLOCK = capi.WFM_COV_SCAN_BLOCK
SPANS = capi.WFM_COV_SPANS


# ---- 1. the ABI against the model ----
def _add(cov, problems, junk=0):
    """problems = [(base, [(length, op)])] in one wfm_coverage_add call; junk: unused words between the problems' runs"""
    probs, words = [], []
    for base, runs in problems:
        words += [0] * junk
        probs.append((base, len(words), len(runs)))
        words += V.words(runs)
    return cov.add(probs, words)


def _entries(cov):
    e = cov.export()
    assert e.dtype.itemsize == 16 and not e["pad_"].any()
    return list(zip(e["pos"].tolist(), e["delta"].tolist()))


def _intervals(cov):
    iv, totals = cov.intervals()
    assert iv.dtype.itemsize == 16 and not iv["pad_"].any()
    return list(zip(iv["start"].tolist(), iv["depth"].tolist())), totals


def _assert_model(cov, problems, n_bases):
    """export and intervals of the object equal the model's for `problems`, word for word"""
    assert _entries(cov) == V.entries_of(problems, n_bases)
    assert _intervals(cov) == V.intervals_of(problems, n_bases)


def _fresh(gpu, problems, n_bases):
    cov = gpu.coverage(n_bases)
    try:
        flags = _add(cov, problems)
        assert not flags.any()
        _assert_model(cov, problems, n_bases)
        return _entries(cov), _intervals(cov)
    finally:
        cov.close()


P = V.parse
HAND = [
    ("ends_on_the_last_word", 5, [(0, P("5="))]),
    ("alternation_is_one_interval", 40, [(3, P("3=1X2=1X4=2X1=1X5="))]),
    ("leading_gaps", 30, [(2, P("2I3D4=")), (12, P("3D2I4="))]),
    ("trailing_gaps", 30, [(2, P("4=3D2I")), (12, P("4=2I3D"))]),
    ("end_to_start", 30, [(2, P("6=")), (8, P("3X2=")), (13, P("1="))]),
    ("three_times", 20, [(4, P("3=2D1I3="))] * 3),
    ("deletion_and_insertion", 20, [(1, P("3=2D3=2I1X"))]),
]


@pytest.mark.parametrize("name,n_bases,problems", HAND, ids=[h[0] for h in HAND])
def test_hand_cases_word_for_word(gpu, name, n_bases, problems):
    entries, (iv, totals) = _fresh(gpu, problems, n_bases)
    if name == "ends_on_the_last_word":
        assert entries == [(0, 1), (5, -1)] and iv == [(0, 1)] and totals == (5, 5, 1)
    if name == "alternation_is_one_interval":
        assert entries == [(3, 1), (23, -1)] and iv == [(0, 0), (3, 1), (23, 0)]
    if name == "end_to_start":
        assert entries == [(2, 1), (14, -1)] and totals == (12, 12, 1)
    if name == "three_times":
        assert iv == [(0, 0), (4, 3), (7, 0), (9, 3), (12, 0)] and totals == (6, 18, 3)
    if name == "deletion_and_insertion":
        assert iv == [(0, 0), (1, 1), (4, 0), (6, 1), (10, 0)]


def _separated(n_runs):
    """n_runs runs: =/X runs with a D between each two"""
    runs = []
    for k in range(n_runs):
        runs.append((1 + k % 3, "D") if k % 2 else (1 + k % 4, "=X"[(k // 2) % 2]))
    return runs


@pytest.mark.parametrize("n_runs", [255, 256, 257, 513])
def test_run_counts_on_the_round_carry(gpu, n_runs):
    runs = _separated(n_runs)
    span = sum(n for n, op in runs)
    # two of them in one call, the second one right behind an unrelated neighbour
    problems = [(7, runs), (7 + span + 5, P("4=")), (7 + span + 20, runs[::-1])]
    _fresh(gpu, problems, 7 + 2 * span + 40)


def test_twenty_thousand_runs(gpu):
    runs = P("1=1D") * 10000
    entries, (iv, totals) = _fresh(gpu, [(0, runs)], 20000)
    assert len(entries) == 20000 > 4 * BLOCK and totals == (10000, 10000, 1)


def test_chunks_of_one_tile(gpu, monkeypatch):
    """the list brought down, and the intervals taken, in chunks of 64 KiB: the depth and the position carried from chunk to chunk"""
    runs = P("1=1D") * 10000
    problems = [(0, runs), (3, P("19000=")), (5000, P("3X"))]
    want = _fresh(gpu, problems, 20000)
    monkeypatch.setenv("WFM_COV_OUT_MB", "0.0625")
    assert 20000 // TILE >= 4  # several chunks
    assert _fresh(gpu, problems, 20000) == want


def test_events_around_the_tile_edges(gpu):
    n_bases = 3 * TILE  # three tiles and the last word in a fourth
    problems = []
    for edge in (TILE, 2 * TILE, 3 * TILE):
        problems += [(edge - 1, P("1=")), (edge - 4, P("2X"))]
        if edge < n_bases:
            problems += [(edge, P("3=")), (edge, P("3=")), (edge + 1, P("2="))]
    entries, _ = _fresh(gpu, problems, n_bases)
    pos = [p for p, _ in entries]
    assert {TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE - 1, 3 * TILE} <= set(pos)
    # each event alone, at the three places, in an object of its own
    for at in (TILE - 1, TILE, TILE + 1):
        e, (iv, totals) = _fresh(gpu, [(at, P("1="))], n_bases)
        assert e == [(at, 1), (at + 1, -1)] and iv == [(0, 0), (at, 1), (at + 1, 0)] and totals == (1, 1, 1)


@pytest.mark.parametrize("count", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1])
def test_nonzero_count_on_the_scan_block(gpu, count):
    """isolated bases give two non-zero words each; two records that share their start give three"""
    problems, at = [], 10
    if count % 2:
        problems += [(at, P("2=")), (at, P("1="))]
        at += 10
    while 2 * len(problems) - (1 if count % 2 else 0) < count:
        problems.append((at, P("1X")))
        at += 3
    entries, _ = _fresh(gpu, problems, at + 10)
    assert len(entries) == count


def test_empty_object_and_no_problems(gpu):
    for n_bases in (0, 1, 5, TILE - 1, TILE, TILE + 1):
        cov = gpu.coverage(n_bases)
        try:
            assert len(cov.add([], [])) == 0  # no problems: WFM_OK
            assert _entries(cov) == [] and _intervals(cov) == ([(0, 0)], (0, 0, 0))
            cov.import_entries(np.zeros(0, dtype=capi.COV_ENTRY_DTYPE))
            assert _entries(cov) == []
        finally:
            cov.close()


def test_spans_are_flagged_and_add_nothing(gpu):
    n_bases = 1000
    good = [(10, P("20=3D5X")), (990, P("10="))]
    cov = gpu.coverage(n_bases)
    try:
        _add(cov, good)
        before = _entries(cov)
        bad = [(991, P("10=")),               # one base past the end
               (995, P("2=4D")),              # its D run leaves
               (n_bases + 1, P("2I")),        # begins behind the last word
               (2 ** 40, P("1=")),
               (500, P("300=") + P("300X") * 2),
               (0, P("5="))]                  # this one is fine
        flags = _add(cov, bad)
        assert flags.tolist() == [SPANS, SPANS, SPANS, SPANS, SPANS, 0]
        assert _entries(cov) == V.entries_of(good + [bad[-1]], n_bases)
        assert [e for e in _entries(cov) if e[0] >= 10] == [e for e in before if e[0] >= 10]
        # a run of length 0 (a word that is nothing but an op) refuses its problem too
        flags = cov.add([(100, 0, 3)], [4 << 2, 1, 4 << 2])
        assert flags.tolist() == [SPANS] and _entries(cov) == V.entries_of(good + [bad[-1]], n_bases)
        # n_bases itself is a legal base for a problem without pattern bases
        assert _add(cov, [(n_bases, P("3I"))]).tolist() == [0]
    finally:
        cov.close()


def test_bad_run_range_and_bad_import(gpu):
    cov = gpu.coverage(100)
    try:
        _add(cov, [(5, P("10="))])
        for probs in ([(0, 2, 3)], [(0, 5, 0)], [(0, 0, 1), (0, 2 ** 40, 1)]):
            with pytest.raises(capi.WfmError, match="leave the run buffer"):
                cov.add(probs, [4 << 2] * 4)
        assert _entries(cov) == [(5, 1), (15, -1)]  # nothing was added, and the handle goes on
        with pytest.raises(capi.WfmError, match="beyond"):
            cov.import_entries(np.array([(3, 1, 0), (101, -1, 0)], dtype=capi.COV_ENTRY_DTYPE))
        assert _entries(cov) == [(5, 1), (15, -1)]
        _add(cov, [(15, P("5="))])
        _assert_model(cov, [(5, P("15="))], 100)
    finally:
        cov.close()


def test_budget_refuses_create(gpu, monkeypatch):
    monkeypatch.setenv("WFM_COV_GB", "0")
    with pytest.raises(capi.WfmError, match=r"GiB.*WFM_COV_GB"):
        gpu.coverage(1000)
    monkeypatch.setenv("WFM_COV_GB", "0.00001")  # 10 KiB
    gpu.coverage(2000).close()
    with pytest.raises(capi.WfmError, match=r"needs 0\.00\d+ GiB"):
        gpu.coverage(1 << 20)
    monkeypatch.delenv("WFM_COV_GB")
    gpu.coverage(1 << 20).close()


# ---- 2. fuzz ----
N_FUZZ = 200003


def _fuzz_problems():
    rng = random.Random(0xC0FE)
    out = []
    for k in range(300):
        runs, last = [], None
        for _ in range(rng.choice([1, 2, 5, 40, 300])):
            op = rng.choice([o for o in "=XID" if o != last])
            runs.append((rng.choice([1, 1, 2, 7, 60, 900]), op))
            last = op
        span = sum(n for n, op in runs if op != "I")
        if span > N_FUZZ:
            runs, span = [(N_FUZZ, "=")], N_FUZZ
        # some at the very ends of the array, some on top of each other
        base = rng.choice([0, N_FUZZ - span, rng.randrange(0, N_FUZZ - span + 1), (k * 977) % (N_FUZZ - span + 1)])
        out.append((base, runs))
    return out


@pytest.fixture(scope="module")
def fuzz():
    problems = _fuzz_problems()
    return types.SimpleNamespace(problems=problems, entries=V.entries_of(problems, N_FUZZ), intervals=V.intervals_of(problems, N_FUZZ))


def test_fuzz_equals_the_model(gpu, fuzz):
    cov = gpu.coverage(N_FUZZ)
    try:
        assert not _add(cov, fuzz.problems, junk=3).any()
        assert _entries(cov) == fuzz.entries and len(fuzz.entries) > 4 * BLOCK
        first, second = cov.intervals(), cov.intervals()
        assert first[0].tobytes() == second[0].tobytes() and first[1] == second[1]  # two calls, the same bytes
        assert _intervals(cov) == fuzz.intervals and fuzz.intervals[1][2] >= 3
        assert cov.export().tobytes() == cov.export().tobytes()
    finally:
        cov.close()


def test_fuzz_in_reverse_order_and_three_calls(gpu, fuzz):
    cov = gpu.coverage(N_FUZZ)
    try:
        rev = fuzz.problems[::-1]
        for part in (rev[:7], rev[7:150], rev[150:]):
            assert not _add(cov, part).any()
        assert _entries(cov) == fuzz.entries and _intervals(cov) == fuzz.intervals
    finally:
        cov.close()


def test_fuzz_split_over_two_objects_and_merged(gpu, fuzz):
    h2 = capi.Handle(0)
    a, b = gpu.coverage(N_FUZZ), h2.coverage(N_FUZZ)
    try:
        _add(a, fuzz.problems[0::2])
        _add(b, fuzz.problems[1::2])
        half = b.export()
        assert list(zip(half["pos"].tolist(), half["delta"].tolist())) == V.entries_of(fuzz.problems[1::2], N_FUZZ)
        a.import_entries(half)
        assert _entries(a) == fuzz.entries and _intervals(a) == fuzz.intervals
        # importing what an object holds with the signs turned empties it
        own = a.export().copy()
        own["delta"] = -own["delta"]
        a.import_entries(own)
        assert _entries(a) == [] and _intervals(a) == ([(0, 0)], (0, 0, 0))
    finally:
        a.close()
        b.close()
        h2.close()


# ---- 3. the align driver ----
def _align(handles, case, out, bg, left=False, **params):
    capi.set_coverage(bg)
    capi.set_left_align(left)
    try:
        if len(handles) == 1:
            capi.align_paf(handles[0], case.fa, case.paf, out, params=params or None)
        else:
            capi.align_paf_multi(handles, case.fa, case.paf, out, params=params or None)
        return open(out, "rb").read(), (open(bg).read() if bg else None), capi.coverage_counts()
    finally:
        capi.set_coverage(None)
        capi.set_left_align(False)


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows, the aligned PAF of a run without the switch and the bedGraph of one with it: made once, never changed"""
    d = str(tmp_path_factory.mktemp("coverage"))
    fa, paf, seqs = LT._make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, seqs=seqs, names=list(seqs), lengths=[len(s) for s in seqs.values()])
    c.text, none, counts = _align([gpu], c, os.path.join(d, "plain.paf"), None)
    assert none is None and counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20
    c.bg_path = os.path.join(d, "plain.bg")
    c.with_text, c.bg, c.counts = _align([gpu], c, os.path.join(d, "with.paf"), c.bg_path)
    return c


def _assert_file(case, problems, aligned, n_records, bg, counts):
    """the bedGraph is the model's for the problems of the lines written, tiles every sequence, and the counts obey the conservation law"""
    depth = V.depth_of(problems, sum(case.lengths))
    assert bg == V.bedgraph(case.names, case.lengths, depth)
    back, n_lines = V.parse_bedgraph(bg, case.names, case.lengths)  # (asserts the tiling)
    assert back.tolist() == depth.tolist()
    assert counts == (n_records, int(np.count_nonzero(depth)), int(depth.sum()), n_lines)
    assert counts[2] == aligned  # the sum of depth is the total of the = and X run lengths of the lines written
    return depth


def test_driver_plain(gpu, case):
    assert case.with_text == case.text
    problems, aligned = V.problems_of_paf(case.lines, case.names, case.lengths)
    depth = _assert_file(case, problems, aligned, len(case.lines), case.bg, case.counts)
    assert depth.max() >= 2 and (depth == 0).any()  # overlapping records and uncovered stretches are both there
    # the switch off again: the bytes of the run without it, no counts, no file
    again, none, counts = _align([gpu], case, os.path.join(case.dir, "off.paf"), None)
    assert again == case.text and none is None and counts == (0, 0, 0, 0)


def test_driver_with_left_align(gpu, case):
    plain, _, _ = _align([gpu], case, os.path.join(case.dir, "la0.paf"), None, left=True)
    text, bg, counts = _align([gpu], case, os.path.join(case.dir, "la.paf"), os.path.join(case.dir, "la.bg"), left=True)
    assert text == plain != case.text
    lines = text.decode().splitlines()
    problems, aligned = V.problems_of_paf(lines, case.names, case.lengths)
    _assert_file(case, problems, aligned, len(lines), bg, counts)
    assert bg != case.bg  # the normalised runs are counted: a deletion that moved uncovers other bases


def test_driver_sam(gpu, case):
    plain, _, _ = _align([gpu], case, os.path.join(case.dir, "s0.sam"), None, sam_format=1)
    text, bg, counts = _align([gpu], case, os.path.join(case.dir, "s.sam"), os.path.join(case.dir, "s.bg"), sam_format=1)
    assert text == plain
    records = [l for l in text.decode().splitlines() if not l.startswith("@")]
    problems, aligned = V.problems_of_sam(records, case.names, case.lengths)
    _assert_file(case, problems, aligned, len(records), bg, counts)
    assert bg == case.bg  # the same records as the PAF's


def test_driver_with_resident_sequences(gpu, case):
    text, bg, counts = _align([gpu], case, os.path.join(case.dir, "r.paf"), os.path.join(case.dir, "r.bg"), resident_sequences=1)
    assert text == case.text and bg == case.bg and counts == case.counts


def test_driver_two_handles_on_one_device(gpu, case):
    h2 = capi.Handle(0)
    try:
        text, bg, counts = _align([gpu, h2], case, os.path.join(case.dir, "m.paf"), os.path.join(case.dir, "m.bg"))
    finally:
        h2.close()
    assert text == case.text
    problems, aligned = V.problems_of_paf(text.decode().splitlines(), case.names, case.lengths)
    _assert_file(case, problems, aligned, len(case.lines), bg, counts)
    assert bg == case.bg and counts == case.counts


def test_driver_filtered_records_add_nothing(gpu, case):
    plain, _, _ = _align([gpu], case, os.path.join(case.dir, "f0.paf"), None, min_alignment_length=5000)
    text, bg, counts = _align([gpu], case, os.path.join(case.dir, "f.paf"), os.path.join(case.dir, "f.bg"), min_alignment_length=5000)
    lines = text.decode().splitlines()
    assert text == plain and 0 < len(lines) < len(case.lines)
    problems, aligned = V.problems_of_paf(lines, case.names, case.lengths)
    _assert_file(case, problems, aligned, len(lines), bg, counts)


# ---- 4. the command line ----
def _cli(args, cwd=None):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "120", CLI] + args, capture_output=True, text=True, cwd=cwd)


COUNTS = r"\[wfmash::coverage\] (\d+) records added, (\d+) bases covered, sum of depth (\d+), (\d+) intervals written"
PAF_COUNTS = r"\[wfmash::coverage\] (\d+) lines added, (\d+) skipped \((\d+) without an =XID cg:Z:, (\d+) malformed, (\d+) with an unknown target, (\d+) with another tlen\), (\d+) bases covered, sum of depth (\d+), max depth (\d+), (\d+) intervals"


def test_cli_beside_the_other_switches_and_from_the_paf(case):
    out, bg, vcf = os.path.join(case.dir, "cli.paf"), os.path.join(case.dir, "cli.bg"), os.path.join(case.dir, "cli.vcf")
    r = _cli(["--coverage", bg, "--variants", vcf, "--cs", "--verify", "-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    lines = open(out).read().splitlines()
    assert [l.rpartition("\tcs:Z:")[0] for l in lines] == case.lines
    assert open(bg).read() == case.bg
    m = re.search(COUNTS, r.stderr)
    assert m and tuple(int(x) for x in m.groups()) == case.counts
    # the file again from the PAF the run wrote, byte for byte
    bg2 = os.path.join(case.dir, "cli2.bg")
    r = _cli(["--coverage-paf", out, "--coverage", bg2, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert open(bg2).read() == case.bg
    m = re.search(PAF_COUNTS, r.stderr)
    got = tuple(int(x) for x in m.groups())
    depth, _ = V.parse_bedgraph(case.bg, case.names, case.lengths)
    assert got == (len(lines), 0, 0, 0, 0, 0, case.counts[1], case.counts[2], int(depth.max()), case.counts[3])


def test_cli_coverage_paf_skips_and_counts(case):
    lines = list(case.lines)
    f = lines[2].split("\t")
    lines[2] = "\t".join(x for x in f if not x.startswith("cg:Z:"))
    f = lines[5].split("\t")
    f[5] = "nobody#1#chrZ"
    lines[5] = "\t".join(f)
    mutated, bg = os.path.join(case.dir, "mut.paf"), os.path.join(case.dir, "mut.bg")
    with open(mutated, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    r = _cli(["--coverage-paf", mutated, "--coverage", bg, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    kept = [l for k, l in enumerate(case.lines) if k not in (2, 5)]
    problems, aligned = V.problems_of_paf(kept, case.names, case.lengths)
    depth = V.depth_of(problems, sum(case.lengths))
    text = open(bg).read()
    assert text == V.bedgraph(case.names, case.lengths, depth)
    m = re.search(PAF_COUNTS, r.stderr)
    got = tuple(int(x) for x in m.groups())
    assert got == (len(kept), 2, 1, 0, 1, 0, int(np.count_nonzero(depth)), aligned, int(depth.max()), text.count("\n"))
    assert int(depth.sum()) == aligned
