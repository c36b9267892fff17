"""GPU tests of --pav: wfm_pav_* through capi, every result held word for word against the brute force of tests/pav_model.py; then the
align driver on the synthetic pangenome of tests/test_left_align_gpu.py and the command line."""
import os
import random
import subprocess
import types

import numpy as np
import pytest

from tests import pav_model as M
from tests import coverage_model as V
from tests import test_left_align_gpu as LT  # its synthetic pangenome (nothing of it is collected from here)
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
BLOCK = capi.WFM_PAV_SCAN_BLOCK
SPANS = capi.WFM_PAV_SPANS
P = M.parse


# ---- 1. the ABI against the model ----
def _add(pav, problems, junk=0):
    """problems = [(base, [(length, op)], group)] in one wfm_pav_add call; junk: unused words between the problems' runs"""
    probs, words = [], []
    for base, runs, g in problems:
        words += [0] * junk
        probs.append((base, len(words), len(runs), g))
        words += M.words(runs)
    return pav.add(probs, words)


def _export(pav):
    e = pav.export()
    assert e.dtype.itemsize == 16
    return list(zip(e["start"].tolist(), e["length"].tolist(), e["group"].tolist()))


def _intervals(n_bases, seed=1):
    """whole, empty, single bases at the edges and a spread of random intervals"""
    rng = random.Random(seed)
    iv = [(0, n_bases), (0, 0), (n_bases, n_bases), (0, min(1, n_bases)), (max(0, n_bases - 1), n_bases)]
    for _ in range(40):
        a = rng.randrange(0, n_bases + 1)
        iv.append((a, min(n_bases, a + rng.choice([0, 1, 2, 5, 17, 300, n_bases]))))
    return iv


def _assert_model(pav, problems, n_bases, n_groups, intervals=None):
    """export and matrix of the object equal the model's for `problems`, word for word; returns both"""
    mask = M.mask_of(problems, n_bases, n_groups)
    iv = intervals if intervals is not None else _intervals(n_bases)
    got_e, got_m = _export(pav), pav.matrix(iv)
    assert got_e == M.union_of(mask)
    assert got_m.shape == (len(iv), n_groups) and got_m.dtype == np.uint32
    assert got_m.tolist() == M.matrix_of(mask, iv)
    return got_e, got_m.tolist()


def _fresh(gpu, problems, n_bases, n_groups, intervals=None):
    pav = gpu.pav(n_bases, n_groups)
    try:
        flags = _add(pav, problems)
        assert not flags.any()
        assert pav.counts()[0] == M.segments_of(problems)
        return _assert_model(pav, problems, n_bases, n_groups, intervals)
    finally:
        pav.close()


HAND = [
    ("leading_gaps", 30, 2, [(2, P("2I3D4="), 0), (12, P("3D2I4="), 1)]),
    ("trailing_gaps", 30, 2, [(2, P("4=3D2I"), 0), (12, P("4=2I3D"), 1)]),
    ("alternation_is_one_segment", 40, 1, [(3, P("3=1X2=1X4=2X1=1X5="), 0)]),
    ("end_to_start", 30, 1, [(2, P("6="), 0), (8, P("3X2="), 0), (13, P("1="), 0)]),
    ("nested_and_overlapping", 60, 1, [(5, P("40="), 0), (10, P("5=3D5="), 0), (30, P("25="), 0), (5, P("40="), 0)]),
    ("same_coordinates_two_groups", 30, 3, [(4, P("10="), 0), (4, P("10="), 2)]),
    ("last_base_then_base_zero", 20, 3, [(15, P("5="), 1), (0, P("5="), 2)]),
    ("inside_a_deletion", 40, 1, [(2, P("5=20D5="), 0)]),
    ("empty_group", 30, 4, [(1, P("5="), 0), (3, P("9="), 3)]),
]


@pytest.mark.parametrize("name,n_bases,n_groups,problems", HAND, ids=[h[0] for h in HAND])
def test_hand_cases_word_for_word(gpu, name, n_bases, n_groups, problems):
    extra = {"end_to_start": [(0, 4), (3, 9), (13, 15)], "inside_a_deletion": [(7, 27), (8, 20), (6, 28), (0, 40)],
             "nested_and_overlapping": [(0, 7), (50, 60), (44, 56)]}.get(name, [])
    iv = _intervals(n_bases) + extra
    union, cells = _fresh(gpu, problems, n_bases, n_groups, iv)
    at = len(iv) - len(extra)
    if name == "alternation_is_one_segment":
        assert union == [(3, 20, 0)]
    if name == "end_to_start":
        assert union == [(2, 12, 0)]
        assert [c[0] for c in cells[at:]] == [2, 6, 1]  # clipped at the left edge, inside, clipped at the right edge
    if name == "nested_and_overlapping":
        assert union == [(5, 50, 0)]
        assert [c[0] for c in cells[at:]] == [2, 5, 11]
    if name == "same_coordinates_two_groups":
        assert union == [(4, 10, 0), (4, 10, 2)] and cells[0] == [10, 0, 10]
    if name == "last_base_then_base_zero":
        assert union == [(15, 5, 1), (0, 5, 2)] and cells[0] == [0, 5, 5]
    if name == "inside_a_deletion":
        assert [c[0] for c in cells[at:]] == [0, 0, 2, 10]
    if name == "empty_group":
        assert cells[0] == [5, 0, 0, 9]


def test_an_interval_clipped_at_both_edges_of_one_union(gpu):
    union, cells = _fresh(gpu, [(10, P("20="), 0), (50, P("5="), 0)], 100, 1, [(12, 25), (5, 35), (10, 30), (29, 51), (0, 100)])
    assert union == [(10, 20, 0), (50, 5, 0)]
    assert [c[0] for c in cells] == [13, 20, 20, 2, 25]


def _separated(n_runs):
    """n_runs runs: =/X runs with a D or an I between each two"""
    runs = []
    for k in range(n_runs):
        runs.append((1 + k % 3, "DI"[(k // 2) % 2]) if k % 2 else (1 + k % 4, "=X"[(k // 2) % 2]))
    return runs


@pytest.mark.parametrize("n_runs", [255, 256, 257, 513])
def test_run_counts_on_the_round_carry(gpu, n_runs):
    runs = _separated(n_runs)
    span = sum(n for n, op in runs if op != "I")
    # two of them in one call, the second one right behind an unrelated neighbour, in another group
    problems = [(7, runs, 0), (7 + span + 5, P("4="), 1), (7 + span + 20, runs[::-1], 1)]
    _fresh(gpu, problems, 7 + 2 * span + 40, 2)


@pytest.mark.parametrize("lead", [250, 255, 256, 506])
def test_a_stretch_across_a_round_boundary_is_one_segment(gpu, lead):
    """`lead` separated runs, then an =/X alternation of 12 runs that straddles run 256 or 512, then more"""
    runs = _separated(lead)
    if runs[-1][1] in "=X":
        runs.append((2, "D"))
    elif runs[-1][1] == "I":  # (behind an insertion the stretch would abut the segment before it)
        runs[-1] = (2, "D")
    stretch = P("3=1X") * 6
    runs = runs + stretch + P("2D5=")
    start = 9 + sum(n for n, op in runs[:len(runs) - len(stretch) - 2] if op != "I")
    pav = gpu.pav(5000, 1)
    try:
        assert not _add(pav, [(9, runs, 0)]).any()
        assert pav.counts()[0] == M.segments_of([(9, runs, 0)])
        union, _ = _assert_model(pav, [(9, runs, 0)], 5000, 1)
        assert (start, 24, 0) in union
    finally:
        pav.close()


def test_twenty_thousand_runs(gpu):
    runs = P("1=1D") * 10000
    union, cells = _fresh(gpu, [(0, runs, 0)], 20000, 1, [(0, 20000), (1, 2), (2, 3), (101, 1100)])
    assert len(union) == 10000 > 4 * BLOCK and [c[0] for c in cells] == [10000, 0, 1, 499]


def _one_per_segment(n_seg, group, step=7, length=3, base=0):
    return [(base + k * step, [(length, "=")], group) for k in range(n_seg)]


@pytest.mark.parametrize("n_seg", [1023, 1024, 1025, 2049])
def test_segment_counts_on_the_scan_blocks(gpu, n_seg):
    n_bases = 7 * n_seg + 10
    problems = _one_per_segment(n_seg, 0)
    union, _ = _fresh(gpu, problems, n_bases, 1)
    assert len(union) == n_seg


@pytest.mark.parametrize("n_seg", [1025, 2049])
def test_the_first_segment_swallows_all_later_ones(gpu, n_seg):
    """the running maximum has to cross every block boundary: the union is ONE interval"""
    n_bases = 7 * n_seg + 10
    problems = [(0, [(n_bases - 1, "=")], 0)] + _one_per_segment(n_seg - 1, 0, base=1)
    union, _ = _fresh(gpu, problems, n_bases, 1)
    assert union == [(0, n_bases - 1, 0)]


def test_three_groups_across_the_scan_blocks(gpu):
    """a swallowing first segment in each of three groups, the groups' borders inside blocks: a group's maximum must not leak into the next"""
    n_bases = 7 * 900 + 10
    problems = []
    for g in range(3):
        problems += [(g, [(3000 + g, "=")], g)] + _one_per_segment(899, g, base=5)
    union, cells = _fresh(gpu, problems, n_bases, 3)
    assert [(u[0], u[2]) for u in union if u[0] < 5] == [(0, 0), (1, 1), (2, 2)] and union[0] == (0, 3000, 0)
    assert len(union) > BLOCK and min(cells[0]) > 3000


def test_flagged_problems_add_nothing(gpu):
    n_bases, n_groups = 100, 2
    good = [(10, P("5=2D5="), 0), (60, P("8="), 1)]
    bad = [(95, P("10="), 0),            # leaves the target
           (101, P("1="), 0),            # begins beyond it
           (20, [(3, "="), (0, "D"), (3, "=")], 0),  # an empty run
           (20, P("5="), 2),             # a group out of range
           (20, P("5="), 0xffffffff)]
    problems = [good[0], bad[0], bad[1], bad[2], good[1], bad[3], bad[4]]
    pav = gpu.pav(n_bases, n_groups)
    try:
        flags = _add(pav, problems, junk=3)
        assert flags.tolist() == [0, SPANS, SPANS, SPANS, 0, SPANS, SPANS]
        assert pav.counts()[0] == M.segments_of(good)
        _assert_model(pav, good, n_bases, n_groups)
    finally:
        pav.close()


def test_a_span_beyond_32_bits_is_flagged(gpu):
    n_bases = (1 << 33) + 100
    pav = gpu.pav(n_bases, 1)
    try:
        long_run = [((1 << 30) - 1, "=")] * 4 + [(4, "=")]  # 2^32 bases
        flags = _add(pav, [(5, long_run, 0), ((1 << 33) + 10, P("7=3D7="), 0), (3, P("4="), 0)])
        assert flags.tolist() == [SPANS, 0, 0]
        assert _export(pav) == [(3, 4, 0), ((1 << 33) + 10, 7, 0), ((1 << 33) + 20, 7, 0)]
        got = pav.matrix([(0, 100), (1 << 33, (1 << 33) + 100), ((1 << 33) + 12, (1 << 33) + 22)])
        assert got.tolist() == [[4], [14], [7]]
    finally:
        pav.close()


def _random_problems(seed, n, n_bases, n_groups):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        runs = []
        for _ in range(rng.randrange(1, 12)):
            runs.append((rng.randrange(1, 30), rng.choice("==XID")))
        span = sum(k for k, op in runs if op != "I")
        out.append((rng.randrange(0, n_bases - span), runs, rng.randrange(n_groups)))
    return out


@pytest.fixture(scope="module")
def random_case():
    n_bases, n_groups = 6000, 5  # group 4 is left empty
    problems = _random_problems(7, 700, n_bases, n_groups - 1)
    mask = M.mask_of(problems, n_bases, n_groups)
    iv = _intervals(n_bases, seed=3)
    return types.SimpleNamespace(n_bases=n_bases, n_groups=n_groups, problems=problems, iv=iv, union=M.union_of(mask), cells=M.matrix_of(mask, iv))


def _feed(gpu, case, calls):
    """a fresh object fed the problems in the given calls; returns (export, matrix, counts)"""
    pav = gpu.pav(case.n_bases, case.n_groups)
    try:
        for c in calls:
            assert not _add(pav, c).any()
        return _export(pav), pav.matrix(case.iv).tolist(), pav.counts()
    finally:
        pav.close()


def test_order_of_problems_and_calls(gpu, random_case):
    c = random_case
    one = _feed(gpu, c, [c.problems])
    assert one[0] == c.union and one[1] == c.cells
    split = _feed(gpu, c, [c.problems[:100], c.problems[100:101], c.problems[101:]])
    rev = _feed(gpu, c, [c.problems[::-1]])
    assert split[:2] == one[:2] and rev[:2] == one[:2]
    assert one[2][0] == split[2][0] == rev[2][0] == M.segments_of(c.problems)


def test_union_twice_is_union_once(gpu, random_case):
    c = random_case
    pav = gpu.pav(c.n_bases, c.n_groups)
    try:
        _add(pav, c.problems)
        pav.union()
        first = (_export(pav), pav.matrix(c.iv).tolist(), pav.counts()[1])
        pav.union()
        pav.union()
        assert (_export(pav), pav.matrix(c.iv).tolist(), pav.counts()[1]) == first
        assert first[0] == c.union and first[2] == len(c.union)
        # ... and a union of the union with itself
        pav.import_(pav.export())
        assert (_export(pav), pav.matrix(c.iv).tolist(), pav.counts()[1]) == first
    finally:
        pav.close()


def test_compaction_after_every_call(gpu, random_case, monkeypatch):
    c = random_case
    monkeypatch.setenv("WFM_PAV_MB", "0")
    calls = [c.problems[k:k + 70] for k in range(0, len(c.problems), 70)]
    got = _feed(gpu, c, calls)
    assert got[0] == c.union and got[1] == c.cells
    assert got[2][2] == len(calls)  # a union behind every add; export found the list clean
    monkeypatch.delenv("WFM_PAV_MB")
    assert _feed(gpu, c, calls)[2][2] == 1


def test_merge_of_two_objects(gpu, random_case):
    c = random_case
    a, b = gpu.pav(c.n_bases, c.n_groups), gpu.pav(c.n_bases, c.n_groups)
    try:
        _add(a, c.problems[:300])
        _add(b, c.problems[300:])
        part = b.export()
        assert len(part)
        a.import_(part)
        assert _export(a) == c.union and a.matrix(c.iv).tolist() == c.cells
        a.import_(np.zeros(0, dtype=capi.PAV_SEG_DTYPE))
        assert _export(a) == c.union
    finally:
        a.close()
        b.close()


def test_matrix_in_chunks(gpu, random_case, monkeypatch, capfd):
    c = random_case
    pav = gpu.pav(c.n_bases, c.n_groups)
    try:
        _add(pav, c.problems)
        monkeypatch.setenv("WFM_PAV_OUT_MB", "0.0001")  # 104 bytes: five rows of five groups
        monkeypatch.setenv("WFM_DEBUG", "1")
        got = pav.matrix(c.iv).tolist()
        monkeypatch.delenv("WFM_DEBUG")
        assert got == c.cells
        err = capfd.readouterr().err
        assert "in %d chunks" % ((len(c.iv) + 4) // 5) in err, err
        monkeypatch.setenv("WFM_PAV_OUT_MB", "0")  # one row at least
        assert pav.matrix(c.iv).tolist() == c.cells
    finally:
        pav.close()


def test_refusals_are_argument_errors(gpu):
    with pytest.raises(capi.WfmError, match="2\\^40"):
        gpu.pav(1 << 40, 1)
    with pytest.raises(capi.WfmError, match="2\\^24"):
        gpu.pav(100, 1 << 24)
    pav = gpu.pav((1 << 40) - 1, (1 << 24) - 1)
    try:
        with pytest.raises(capi.WfmError, match="2\\^32"):
            pav.matrix([(0, 1 << 32)])
        with pytest.raises(capi.WfmError, match="interval 1"):
            pav.matrix([(0, 5), (7, 6)])
        with pytest.raises(capi.WfmError, match="interval 0"):
            pav.matrix([(5, 1 << 40)])
        with pytest.raises(capi.WfmError, match="segment 0"):
            pav.import_(np.array([(5, 0, 0)], dtype=capi.PAV_SEG_DTYPE))
        with pytest.raises(capi.WfmError, match="segment 1"):
            pav.import_(np.array([(5, 1, 0), (5, 1, (1 << 24) - 1)], dtype=capi.PAV_SEG_DTYPE))
        with pytest.raises(capi.WfmError, match="leave the run buffer"):
            pav.add([(0, 2, 5, 0)], [4, 4, 4])
        assert pav.counts() == (0, 0, 0) and len(pav.export()) == 0
        # the handle and the object stay usable; the largest legal group and the last base
        assert not pav.add([((1 << 40) - 6, 0, 1, (1 << 24) - 2)], M.words(P("5="))).any()
        assert _export(pav) == [((1 << 40) - 6, 5, (1 << 24) - 2)]
        assert pav.matrix([((1 << 40) - 3, (1 << 40) - 1)])[0, (1 << 24) - 2] == 2
    finally:
        pav.close()


# ---- 2. the align driver ----
def _align(handles, case, out, bed, window, pav_out, left=False, coverage=None, fa=None, query_fa=None, paf=None, **params):
    capi.set_pav(bed, window, pav_out)
    capi.set_left_align(left)
    capi.set_coverage(coverage)
    try:
        args = (fa or case.fa, paf or case.paf, out)
        if len(handles) == 1:
            capi.align_paf(handles[0], *args, query_fasta=query_fa, params=params or None)
        else:
            capi.align_paf_multi(handles, *args, query_fasta=query_fa, params=params or None)
        return open(out, "rb").read(), (open(pav_out).read() if pav_out else None), capi.pav_counts()
    finally:
        capi.set_pav(None, 0, None)
        capi.set_left_align(False)
        capi.set_coverage(None)


def _bed_of(names, lengths):
    """1 kb windows tiling every sequence, a few nested genes, one interval over a whole sequence, and lines to skip"""
    out = ["# genes", "track name=x"]
    for name, n in zip(names, lengths):
        out += ["%s\t%d\t%d\tw%d" % (name, a, min(n, a + 1000), a // 1000) for a in range(0, n, 1000)]
        out += ["%s\t0\t%d" % (name, n), "%s\t1990\t2060\trepeat\t0\t-" % name, "%s\t2000\t2004\ttiny" % name, "%s\t%d\t%d\tbeyond" % (name, n - 1, n + 1)]
    out += ["nobody#1#chrZ\t0\t10\tunknown", ""]
    return "\n".join(out) + "\n"


def _intervals_of_bed(text, names, lengths):
    """what lift::parse_bed keeps of _bed_of's lines, in the file's order: sorted by (global start, end, input order)"""
    off, kept = M.offsets(lengths), []
    for line in text.splitlines():
        f = line.split("\t")
        if len(f) < 3 or f[0] not in names:
            continue
        c, a, b = names.index(f[0]), int(f[1]), int(f[2])
        if a < b <= lengths[c]:
            kept.append((int(off[c]) + a, int(off[c]) + b, len(kept), c, a, b, f[3] if len(f) > 3 and f[3] else "."))
    return [(c, a, b, name) for _, _, _, c, a, b, name in sorted(kept)]


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows, a BED over it, the aligned PAF of a run without the switch and the table of one with it: made once,
    never changed"""
    d = str(tmp_path_factory.mktemp("pav"))
    fa, paf, seqs = LT._make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, seqs=seqs, names=list(seqs), lengths=[len(s) for s in seqs.values()])
    c.cols = M.columns(c.names)
    assert c.cols == ["hap0#1", "hap1#1", "hap2#1", "hap3#1", "hap9#1"]
    c.bed = os.path.join(d, "genes.bed")
    bed_text = _bed_of(c.names, c.lengths)
    with open(c.bed, "w") as f:
        f.write(bed_text)
    c.intervals = _intervals_of_bed(bed_text, c.names, c.lengths)
    c.bed_skipped = 4 + len(c.names)
    c.text, none, counts = _align([gpu], c, os.path.join(d, "plain.paf"), None, 0, None)
    assert none is None and counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20
    c.with_text, c.table, c.counts = _align([gpu], c, os.path.join(d, "with.paf"), c.bed, 0, os.path.join(d, "with.pav"))
    return c


def _want(case, lines, intervals=None):
    return M.file_of(case.names, case.lengths, case.cols, intervals or case.intervals, M.problems_of_paf(lines, case.names, case.lengths, case.cols))


def test_driver_plain(gpu, case):
    assert case.with_text == case.text  # the PAF is byte-identical with and without --pav
    assert case.table == _want(case, case.lines)
    assert case.counts[0] == len(case.lines) and case.counts[1] == len(case.intervals) and case.counts[3] == case.bed_skipped
    rows = [l.split("\t") for l in case.table.splitlines()[1:]]
    cells = np.array([[int(x) for x in r[5:]] for r in rows])
    assert (cells > 0).any() and (cells == 0).any() and all(cells[j].max() <= int(r[4]) for j, r in enumerate(rows))
    # the switch off again: the bytes of the run without it, no counts, no file
    again, none, counts = _align([gpu], case, os.path.join(case.dir, "off.paf"), None, 0, None)
    assert again == case.text and none is None and counts == (0, 0, 0, 0)


def test_driver_threads_and_two_handles(gpu, case):
    text, table, counts = _align([gpu], case, os.path.join(case.dir, "t8.paf"), case.bed, 0, os.path.join(case.dir, "t8.pav"), threads=8)
    assert text == case.text and table == case.table and counts == case.counts
    text, table, counts = _align([gpu], case, os.path.join(case.dir, "t1.paf"), case.bed, 0, os.path.join(case.dir, "t1.pav"), threads=1)
    assert text == case.text and table == case.table and counts == case.counts
    h2 = capi.Handle(0)
    try:
        text, table, counts = _align([gpu, h2], case, os.path.join(case.dir, "m.paf"), case.bed, 0, os.path.join(case.dir, "m.pav"))
    finally:
        h2.close()
    assert text == case.text and table == case.table and counts == case.counts


def test_driver_two_gpus(gpu, case):
    if capi.load().wfm_device_count() < 2:
        pytest.skip("one GPU on this node: the two-GPU file cannot be made")
    h2 = capi.Handle(1)
    try:
        text, table, counts = _align([gpu, h2], case, os.path.join(case.dir, "g2.paf"), case.bed, 0, os.path.join(case.dir, "g2.pav"))
    finally:
        h2.close()
    assert text == case.text and table == case.table and counts == case.counts


def test_driver_with_left_align(gpu, case):
    plain, _, _ = _align([gpu], case, os.path.join(case.dir, "la0.paf"), None, 0, None, left=True)
    text, table, _ = _align([gpu], case, os.path.join(case.dir, "la.paf"), case.bed, 0, os.path.join(case.dir, "la.pav"), left=True)
    assert text == plain != case.text
    assert table == _want(case, text.decode().splitlines())  # the normalised runs count


def test_driver_filtered_records_add_nothing(gpu, case):
    text, table, counts = _align([gpu], case, os.path.join(case.dir, "f.paf"), case.bed, 0, os.path.join(case.dir, "f.pav"), min_alignment_length=5000)
    lines = text.decode().splitlines()
    assert 0 < len(lines) < len(case.lines) and counts[0] == len(lines)
    assert table == _want(case, lines) != case.table


def test_driver_windows(gpu, case):
    text, table, counts = _align([gpu], case, os.path.join(case.dir, "w.paf"), None, 3000, os.path.join(case.dir, "w.pav"))
    wins = [(c, a, b, ".") for c, a, b in M.windows(case.names, case.lengths, 3000)]
    assert text == case.text and table == _want(case, case.lines, wins) and counts[1] == len(wins) and counts[3] == 0
    # the rows tile every sequence, and no cell exceeds its window
    at = {}
    for line in table.splitlines()[1:]:
        f = line.split("\t")
        assert int(f[1]) == at.get(f[0], 0) and f[3] == "." and int(f[4]) == int(f[2]) - int(f[1]) and 0 < int(f[4]) <= 3000
        assert all(0 <= int(x) <= int(f[4]) for x in f[5:])
        at[f[0]] = int(f[2])
    assert at == dict(zip(case.names, case.lengths))


def test_driver_all_three_switches_on_one_run(gpu, case):
    """--coverage, --pav and --lift together pack a batch's records once: the three files and the PAF are, byte for byte, those of three
    runs with one switch each (the run with --pav alone is the fixture's)"""
    d = case.dir

    def run(tag, cov, pav, lift):
        capi.set_lift(case.bed if lift else None, lift)
        try:
            text, table, _ = _align([gpu], case, os.path.join(d, tag + ".paf"), case.bed if pav else None, 0, pav, coverage=cov)
        finally:
            capi.set_lift(None, None)
        return text, table, (open(cov, "rb").read() if cov else None), (open(lift, "rb").read() if lift else None)

    text_c, _, bedgraph, _ = run("only_cov", os.path.join(d, "only.bg"), None, None)
    text_l, _, _, lifts = run("only_lift", None, None, os.path.join(d, "only.lift"))
    text, table, bedgraph3, lifts3 = run("all3", os.path.join(d, "all3.bg"), os.path.join(d, "all3.pav"), os.path.join(d, "all3.lift"))
    assert text == text_c == text_l == case.with_text == case.text
    assert len(bedgraph) > 0 and len(lifts) > 0
    assert bedgraph3 == bedgraph and lifts3 == lifts and table == case.table


def test_pav_paf_entry_point(gpu, case):
    out = os.path.join(case.dir, "offline.pav")
    counts = capi.pav_paf(gpu, case.fa, None, os.path.join(case.dir, "plain.paf"), case.bed, 0, out)
    assert open(out).read() == case.table and counts == case.counts


def test_cross_check_against_coverage(gpu, case):
    """targets and queries in two FASTAs, the queries all of one group: a whole-sequence cell is the bases of that sequence with depth > 0"""
    d = case.dir
    names = case.names
    targets = {"ref#1#a": case.seqs[names[0]], "ref#1#b": case.seqs[names[1]]}
    queries = {"smp#2#x": case.seqs[names[2]], "smp#2#y": case.seqs[names[3]], "smp#2#z": case.seqs[names[1]]}
    tfa, qfa, paf = os.path.join(d, "t.fa"), os.path.join(d, "q.fa"), os.path.join(d, "tq.paf")
    LT._write_fasta(tfa, targets)
    LT._write_fasta(qfa, queries)
    rows, chain = [], 0
    for qn, q in queries.items():
        for tn, t in targets.items():
            for a, b in ((1000, 7000), (5000, 12000), (25000, 31000)):
                chain += 1
                rows.append("\t".join(map(str, [qn, len(q), a, b, "+", tn, len(t), a + 10, b - 10, 100, b - a, 30, "id:f:0.97", "kc:f:0.9", "ch:Z:%d.1.1" % chain])))
    with open(paf, "w") as f:
        f.write("\n".join(rows) + "\n")
    bed = os.path.join(d, "whole.bed")
    tn, tl = list(targets), [len(s) for s in targets.values()]
    with open(bed, "w") as f:
        f.write("".join("%s\t0\t%d\tall\n" % (n, l) for n, l in zip(tn, tl)))
    bg = os.path.join(d, "tq.bg")
    text, table, counts = _align([gpu], case, os.path.join(d, "tq.out.paf"), bed, 0, os.path.join(d, "tq.pav"), coverage=bg, fa=tfa, query_fa=qfa, paf=paf)
    assert len(text.decode().splitlines()) >= 12
    depth, _ = V.parse_bedgraph(open(bg).read(), tn, tl)
    off = M.offsets(tl)
    lines = table.splitlines()
    assert lines[0] == "#tname\ttstart\ttend\tname\tlen\tsmp#2" and len(lines) == 3
    for c in range(2):
        covered = int(np.count_nonzero(depth[off[c]:off[c + 1]]))
        assert lines[1 + c] == "%s\t0\t%d\tall\t%d\t%d" % (tn[c], tl[c], tl[c], covered) and 0 < covered < tl[c]
    assert depth.max() >= 2  # records lie on top of each other: a depth, but one union


# ---- 3. the command line ----
def _cli(args, cwd=None):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "120", CLI] + args, capture_output=True, text=True, cwd=cwd)


def test_cli_beside_the_other_switches_and_from_the_paf(case):
    out, table, bg = os.path.join(case.dir, "cli.paf"), os.path.join(case.dir, "cli.pav"), os.path.join(case.dir, "cli.bg")
    r = _cli(["--pav", case.bed, "--pav-out", table, "--coverage", bg, "--cs", "--verify", "-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    lines = open(out).read().splitlines()
    assert [l.rpartition("\tcs:Z:")[0] for l in lines] == case.lines
    assert open(table).read() == case.table
    assert "[wfmash::pav] %d records added, %d rows written, %d union intervals, %d BED lines skipped" % case.counts in r.stderr
    # the file again from the PAF the run wrote, byte for byte
    table2 = os.path.join(case.dir, "cli2.pav")
    r = _cli(["--pav-paf", out, "--pav", case.bed, "--pav-out", table2, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert open(table2).read() == case.table
    assert "%d lines added, 0 skipped" % len(lines) in r.stderr
    # a line whose query the FASTA does not have is skipped and counted
    f = lines[3].split("\t")
    f[0] = "nobody#1#chrQ"
    mutated = os.path.join(case.dir, "mut.paf")
    with open(mutated, "w") as fh:
        fh.write("\n".join(lines[:3] + ["\t".join(f)] + lines[4:]) + "\n")
    r = _cli(["--pav-paf", mutated, "--pav-window", "3000", "--pav-out", table2, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    wins = [(c, a, b, ".") for c, a, b in M.windows(case.names, case.lengths, 3000)]
    assert open(table2).read() == _want(case, case.lines[:3] + case.lines[4:], wins)
    assert "%d lines added, 1 skipped" % (len(lines) - 1) in r.stderr and "1 with an unknown query" in r.stderr


@pytest.mark.parametrize("args, message", [
    (["--pav", "x.bed", "--pav-out", "x.tsv", "--pav-paf", "x.paf", "--left-align"], "--pav-paf runs nothing else"),
])
def test_cli_pav_paf_alone(args, message):
    r = _cli(args + ["t.fa"])
    assert r.returncode == 1 and message in r.stderr
