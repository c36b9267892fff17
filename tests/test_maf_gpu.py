"""--maf on the device: wfm_maf_rows on hand-built problems, at the edges of the write kernel's slices, under split, on odd layouts, in
chunks and on aligned pairs against the rule's model (tests/maf_model.py); then the align driver and the command line."""
import ctypes as C
import gzip
import os
import random
import re
import subprocess
import types

import numpy as np
import pytest

from tests import left_align_model as M
from tests import maf_model as MM
from tests import test_cs_gpu as CT  # its recipe of aligned pairs (nothing of it is collected from here)
from tests import test_left_align_gpu as LT  # its synthetic pangenome (nothing of it is collected from here)
from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
LPA = os.path.join(ROOT, "tests", "golden", "LPA.subset.fa.gz")
RC = bytes.maketrans(b"ACGT", b"TGCA")
UNI = capi.WFM_MODE_END2END_UNI
SLICE = capi.WFM_MAF_SLICE


def _pack(cases):
    """[(P, T, runs)] -> (items for upload, results as tuples, the runs of all problems as words)"""
    items, results, words = [], [], []
    for P, T, runs in cases:
        items.append((P, T, UNI))
        w = M.to_words(runs)
        results.append((0, -1, len(words), sum(n for n, _ in runs), len(w)))
        words += w
    return items, results, np.array(words, dtype=np.uint32)


def _case(cigar, seed=1):
    """(P, T, runs) of a CIGAR over seeded random bases (the rows are spelled from the runs: the bases need not fit them)"""
    runs = M.parse(cigar)
    P = synth.random_dna(seed, sum(n for n, o in runs if o != "I"))
    T = synth.random_dna(seed + 1000, sum(n for n, o in runs if o != "D"))
    return P, T, runs


def _table(blocks):
    return [tuple(int(v) for v in b) for b in blocks.tolist()]


def _per(per):
    return [(c.flags, c.n_runs, c.first, c.count) for c in per]


def _call(gpu, cases, splits=(0,)):
    """{split: (block table as tuples, rows, per as tuples)}, one upload"""
    items, results, words = _pack(cases)
    S = gpu.upload(items)
    try:
        out = {}
        for split in splits:
            blocks, rows, per = gpu.maf_rows(S, results, words, split)
            out[split] = (_table(blocks), rows, _per(per))
        return out
    finally:
        S.free()


def _assert_model(got, cases, name=None):
    for split, (blocks, rows, per) in got.items():
        wb, wr, wp = MM.call_of(cases, split)
        assert per == wp, (name, split)
        assert blocks == wb, (name, split)
        assert rows == wr, (name, split)
        # off is contiguous and the bytes are two rows of every block
        at = 0
        for b in blocks:
            assert b[0] == at, (name, split)
            at += 2 * b[6]
        assert at == len(rows), (name, split)


# ---- 1. hand cases ----
HAND = [
    # name, P, T, CIGAR, row P, row T, (p, t, psize, tsize, cols, eq, x)
    ("m_only", b"ACGTA", b"ACGTA", "5=", b"ACGTA", b"ACGTA", (0, 0, 5, 5, 5, 5, 0)),
    ("x_only_with_n", b"ACT", b"GTN", "3X", b"ACT", b"GTN", (0, 0, 3, 3, 3, 0, 3)),
    ("i_inside", b"ACGT", b"ACNGT", "2=1I2=", b"AC-GT", b"ACNGT", (0, 0, 4, 5, 5, 4, 0)),
    ("i_and_d_inside", b"ACTTGGA", b"ACCAGA", "2=2I3D2=", b"AC--TTGGA", b"ACCA---GA", (0, 0, 7, 6, 9, 4, 0)),
    ("m_over_different_x_over_equal", b"AAGG", b"AATT", "2X2=", b"AAGG", b"AATT", (0, 0, 4, 4, 4, 2, 2)),
    ("i_alone", b"", b"ACGN", "4I", b"----", b"ACGN", (0, 0, 0, 4, 4, 0, 0)),
    ("d_alone", b"TTGA", b"", "4D", b"TTGA", b"----", (0, 0, 4, 0, 4, 0, 0)),
]


def test_hand_cases_byte_for_byte(gpu):
    cases = [(P, T, M.parse(cg)) for _, P, T, cg, _, _, _ in HAND]
    got = _call(gpu, cases)
    blocks, rows, per = got[0]
    want_rows, want_table, want_per = b"", [], []
    for i, (name, _, _, cg, rp, rt, shape) in enumerate(HAND):
        want_table.append((len(want_rows), i) + shape)
        want_per.append((0, len(M.parse(cg)), i, 1))
        want_rows += rp + rt
    assert rows == want_rows
    assert blocks == want_table
    assert per == want_per
    _assert_model(got, cases)


# ---- 2. the edges of a slice ----
NEIGHBOUR = (b"ACG", b"ACT", [(2, "M"), (1, "X")])  # behind every case: an overrun shows in it


def _edge_cases():
    c = {}
    for d in (-1, 0, 1):  # the seam between row P and row T on, before and behind a slice boundary (bytes = 2 cols: the block's end lies on the next)
        c["cols_of_half_a_slice%+d" % d] = "%d=3I2X2D1=" % (SLICE // 2 + d - 8)
    for d in (-1, 0, 1):  # the seam in the middle of a slice, the block's end on, before and behind a boundary
        c["cols_of_a_slice%+d" % d] = "%d=3I2X2D1=" % (SLICE + d - 8)
    c["d_run_across_a_boundary_in_row_t"] = "6380=10D3610="     # cols 10000: row T's '-' are the bytes 16380 .. 16390
    c["i_run_across_a_boundary_in_row_p"] = "16380=10I100="     # row P's '-' are the bytes 16380 .. 16390
    c["d_of_70000"] = "5=70000D5="
    c["m_of_70000"] = "3I70000=2X"
    c["20000_runs"] = "1=1X" * 10000
    c["20000_runs_with_gaps"] = "1=1I1=1D" * 5000
    return c


def _cols(cg):
    return sum(n for n, _ in M.parse(cg))


def test_edge_cases_are_what_their_names_say():
    c = _edge_cases()
    for d in (-1, 0, 1):
        assert _cols(c["cols_of_half_a_slice%+d" % d]) == SLICE // 2 + d and _cols(c["cols_of_a_slice%+d" % d]) == SLICE + d
    (P, T, runs) = _case(c["d_run_across_a_boundary_in_row_t"])
    (_, rt), = MM.rows_of(P, T, runs)
    assert len(rt) == 10000 and rt[SLICE - 10000 - 4:SLICE - 10000 + 6] == b"-" * 10 and rt[SLICE - 10000 - 5] != 45 and rt[SLICE - 10000 + 6] != 45
    (P, T, runs) = _case(c["i_run_across_a_boundary_in_row_p"])
    (rp, _), = MM.rows_of(P, T, runs)
    assert rp[SLICE - 4:SLICE + 6] == b"-" * 10 and rp[SLICE - 5] != 45 and rp[SLICE + 6] != 45


def test_slice_edges(gpu):
    names, cases = [], []
    for k, (name, cg) in enumerate(_edge_cases().items()):
        names += [name, name + ":neighbour"]
        cases += [_case(cg, seed=0xE0 + k), NEIGHBOUR]
    got = _call(gpu, cases)
    _assert_model(got, cases)
    blocks, rows, per = got[0]
    assert len(blocks) == len(cases) and all(p[3] == 1 for p in per)
    for i in range(1, len(cases), 2):  # every neighbour, where an overrun of the case before it would show
        off = blocks[i][0]
        assert rows[off:off + 6] == b"ACGACT", names[i]


def test_slice_edges_each_first_in_the_output(gpu):
    """the same rows where the slices are counted from their own first byte (in test_slice_edges every case lies behind the ones before
    it, at whatever offset they leave)"""
    for k, (name, cg) in enumerate(_edge_cases().items()):
        cases = [_case(cg, seed=0xE0 + k), NEIGHBOUR]
        _assert_model(_call(gpu, cases), cases, name)


# ---- 3. split ----
def test_split_thresholds_on_one_stretch(gpu):
    """2I3D is a stretch of 5 gap bases: a break from N = 4 and N = 5, kept under N = 6; N = 1 breaks at every gap"""
    P, T, runs = b"ACTTGGA", b"ACCAGA", M.parse("2=2I3D2=")
    cases = [(P, T, runs), NEIGHBOUR, _case("4=1I3=2D1X1=1D1I6=", seed=0x51), NEIGHBOUR]
    got = _call(gpu, cases, splits=(1, 4, 5, 6))
    for N in (4, 5):
        blocks, rows, per = got[N]
        assert blocks[:2] == [(0, 0, 0, 0, 2, 2, 2, 2, 0), (4, 0, 5, 4, 2, 2, 2, 2, 0)] and rows[:8] == b"ACACGAGA" and per[0] == (0, 4, 0, 2)
    blocks, rows, per = got[6]
    assert blocks[0] == (0, 0, 0, 0, 7, 6, 9, 4, 0) and rows[:18] == b"AC--TTGGAACCA---GA" and per[0] == (0, 4, 0, 1)
    assert got[1][2][2] == (0, 9, 3, 4)  # 4= | 3= | 1X1= | 6=
    _assert_model(got, cases)


def test_split_breaks_at_the_ends_and_alone(gpu):
    """two breaks with a one-column block between them; a break as the first and as the last run; a problem that is only a break"""
    cases = [_case("5=9D1=4I5D7=", seed=0x52), NEIGHBOUR, _case("6I4=1X", seed=0x53), NEIGHBOUR, _case("4=1X3I3D", seed=0x54), NEIGHBOUR,
             _case("3I3D", seed=0x55), NEIGHBOUR, _case("7D", seed=0x56), NEIGHBOUR]
    got = _call(gpu, cases, splits=(0, 6))
    blocks, rows, per = got[6]
    assert [p[3] for p in per] == [3, 1, 1, 1, 1, 1, 0, 1, 0, 1] and all(p[0] == 0 for p in per)
    assert [b[2:8] for b in blocks[:3]] == [(0, 0, 5, 5, 5, 5), (14, 5, 1, 1, 1, 1), (20, 10, 7, 7, 7, 7)]
    assert blocks[4][2:7] == (0, 6, 5, 5, 5)  # behind the leading break
    assert blocks[6][2:7] == (0, 0, 5, 5, 5)  # before the trailing one
    _assert_model(got, cases)


def test_split_ten_thousand_blocks_in_one_problem(gpu):
    cases = [_case("3=7D" * 10000, seed=0x57), NEIGHBOUR, _case("2X8I" * 300 + "1=", seed=0x58), NEIGHBOUR]
    got = _call(gpu, cases, splits=(7, 8))
    assert got[7][2][0] == (0, 20000, 0, 10000) and got[8][2][0] == (0, 20000, 0, 1)
    assert got[7][2][2][3] == 301 and got[8][2][2][3] == 301
    _assert_model(got, cases)


def test_split_dropped_columns_across_a_slice_boundary(gpu):
    """a break whose columns, had they been written, would have crossed a boundary: the block behind it begins 4 bytes before the boundary;
    and the same with the break in the first row's part of the slice"""
    cases = [_case("8190=10D8190=", seed=0x59), NEIGHBOUR, _case("16380=12I2D300=", seed=0x5A), NEIGHBOUR]
    got = _call(gpu, cases, splits=(0, 10, 15))
    assert [b[0] for b in got[10][0][:2]] == [0, SLICE - 4]
    _assert_model(got, cases)


def test_split_zero_is_one_block(gpu):
    cases = [_case("30=2X1I400=7D3=", seed=3), _case("5=70000D5=", seed=4), NEIGHBOUR]
    blocks, rows, per = _call(gpu, cases)[0]
    assert [p[3] for p in per] == [1, 1, 1]
    for (P, T, runs), b in zip(cases, blocks):
        (rp, rt), = MM.rows_of(P, T, runs, 0)
        assert rows[b[0]:b[0] + 2 * b[6]] == rp + rt and b[6] == sum(n for n, _ in runs)


# ---- 4. layout and refusals ----
def test_reverse_order_with_unused_words(gpu):
    cases = [(P, T, M.parse(cg)) for _, P, T, cg, _, _, _ in HAND] + [_case("30=2X1I400=7D3=", seed=3)]
    items = [(P, T, UNI) for P, T, _ in cases]
    words, results = [], [None] * len(cases)
    for i in reversed(range(len(cases))):
        words += [0xFFFFFFFF] * (1 + i % 3)  # never read
        w = M.to_words(cases[i][2])
        results[i] = (0, -1, len(words), sum(n for n, _ in cases[i][2]), len(w))
        words += w
    words += [0xFFFFFFFF] * 5
    S = gpu.upload(items)
    try:
        got = {}
        for split in (0, 3):
            blocks, rows, per = gpu.maf_rows(S, results, np.array(words, dtype=np.uint32), split)
            got[split] = (_table(blocks), rows, _per(per))
    finally:
        S.free()
    _assert_model(got, cases)


def test_not_done_spans_and_bad_arguments(gpu):
    P, T, runs = _case("20=1X3I30=2D10=", seed=5)
    w = M.to_words(runs)
    short = M.to_words([(runs[0][0] - 1, "M")] + runs[1:])  # one base short of plen
    n_ops = sum(n for n, _ in runs)
    items = [(P, T, UNI | capi.WFM_MODE_SCORE_ONLY), (P, T, UNI), (b"", b"", UNI), (P, T, UNI), (P, T, UNI), (P, T, UNI)]
    words = np.array(w + short + w, dtype=np.uint32)
    # (-300: WFM_ST_UNREACHABLE)
    results = [(0, 27, 0, 0, 0), (-300, -1, 0, n_ops, len(w)), (0, 0, 0, 0, 0), (0, -1, 0, n_ops, len(w)),
               (0, -1, len(w), n_ops - 1, len(short)), (0, -1, 2 * len(w), n_ops, len(w))]
    S = gpu.upload(items)
    try:
        for split in (0, 2):
            rows1 = b"".join(rp + rt for rp, rt in MM.rows_of(P, T, runs, split))
            nb = len(MM.blocks_of(runs, split))
            blocks, rows, per = gpu.maf_rows(S, results, words, split)
            assert [c.flags for c in per] == [capi.WFM_MAF_NOT_DONE] * 3 + [0, capi.WFM_MAF_SPANS, 0]
            assert [c.count for c in per] == [0, 0, 0, nb, 0, nb]
            assert [c.first for c in per] == [0, 0, 0, 0, nb, nb]
            assert rows == rows1 + rows1  # the neighbours of the flagged problem untouched
            assert [int(b["problem"]) for b in blocks] == [3] * nb + [5] * nb
            # the return value: the number of problems flagged WFM_MAF_SPANS
            arr = (capi.Result * len(results))()
            for i, (status, score, ops_off, ops_len, n_runs) in enumerate(results):
                arr[i].status, arr[i].score, arr[i].ops_off, arr[i].ops_len, arr[i].n_runs = status, score, ops_off, ops_len, n_runs
            bp, rp_, nbk, total, pr = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0), (capi.MafCall * len(results))()
            rc = gpu._L.wfm_maf_rows(gpu._p, S._p, arr, words.ctypes.data, len(words), split, C.byref(bp), C.byref(nbk), C.byref(rp_), C.byref(total), pr)
            assert rc == 1 and total.value == 2 * len(rows1) and nbk.value == 2 * nb
            gpu._L.wfm_free_maf(bp, rp_)
            # a run range past the buffer: WFM_E_ARG, the outputs NULL (maf_rows asserts it), and the handle goes on working
            bad = list(results)
            bad[5] = (0, -1, 2 * len(w) + 1, n_ops, len(w))
            with pytest.raises(capi.WfmError, match=r"\(-3\).*leave the run buffer"):
                gpu.maf_rows(S, bad, words, split)
            b2, again, _ = gpu.maf_rows(S, results, words, split)
            assert again == rows and b2.tobytes() == blocks.tobytes()
    finally:
        S.free()


def test_no_problems(gpu):
    S = gpu.upload([])
    try:
        blocks, rows, per = gpu.maf_rows(S, [], np.zeros(0, dtype=np.uint32), 0)
        assert len(blocks) == 0 and rows == b"" and per == []
    finally:
        S.free()


# ---- 5. chunks ----
def test_output_in_chunks_of_one_mib(gpu, monkeypatch):
    """about 3 MB of rows through a 1 MiB output block: problems of 200 kB to 400 kB in chunks of several, one of 1.2 MB in a chunk of
    its own; with split, many blocks a chunk"""
    rng = random.Random(0xC4)
    cases = []
    for k, L in enumerate((100000, 200000, 150000, 600000, 150000, 175000, 100000)):
        parts, left = [], L
        while left > 0:
            m = min(left, rng.randint(1, 20000))
            parts.append("%d=" % m)
            left -= m
            if left > 0:
                parts.append(rng.choice(["1X", "2X", "3I", "40D", "1I", "1D"]))
        cases.append(_case("".join(parts), seed=0xC40 + k))
    items, results, words = _pack(cases)
    S = gpu.upload(items)
    try:
        default = {split: gpu.maf_rows(S, results, words, split) for split in (0, 30)}
        monkeypatch.setenv("WFM_MAF_OUT_MB", "1")
        small = {split: gpu.maf_rows(S, results, words, split) for split in (0, 30)}
    finally:
        S.free()
    assert 2900000 < len(default[0][1]) < 3200000 and len(default[30][0]) > len(cases)
    for split in (0, 30):
        assert small[split][1] == default[split][1] and small[split][0].tobytes() == default[split][0].tobytes()
    _assert_model({split: (_table(b), r, _per(p)) for split, (b, r, p) in small.items()}, cases)


def test_output_of_several_host_copies(gpu):
    """10.2 MB of rows in one chunk: they come down in pieces of 4 MiB, two full ones and a rest, and a problem lies across each of the
    two seams"""
    cases = [_case("%d=1X%d=3I%d=" % (L, L // 2, L // 3), seed=0xB16 + k) for k, L in enumerate((820000, 930000, 1040000))]
    got = _call(gpu, cases)
    blocks, rows, _ = got[0]
    assert 2 * (4 << 20) < len(rows) < 3 * (4 << 20)
    assert blocks[1][0] < (4 << 20) < blocks[2][0] < (8 << 20) < len(rows)
    _assert_model(got, cases)


# ---- 6. fuzz: aligned pairs ----
@pytest.fixture(scope="module")
def fuzz(gpu):
    """the pairs of test_cs_gpu's recipe, aligned once: seqset, results and runs, and the model's answer for split 0 and 50; never changed"""
    items = CT._fuzz_items()
    S = gpu.upload(items)
    failed, words = gpu.align_resident_rle(S)
    assert failed == 0
    runs = [M.from_words(words[S.results[i].ops_off:S.results[i].ops_off + S.results[i].n_runs]) for i in range(S.n)]
    cases = [(it[0], it[1], r) for it, r in zip(items, runs)]
    model = {split: MM.call_of(cases, split) for split in (0, 50)}
    yield types.SimpleNamespace(items=items, S=S, words=words, runs=runs, cases=cases, model=model)
    S.free()


def test_fuzz_equals_the_model_and_undoes(gpu, fuzz):
    for split in (0, 50):
        blocks, rows, per = gpu.maf_rows(fuzz.S, fuzz.S.results, fuzz.words, split)
        assert all(c.flags == 0 for c in per)
        wb, wr, wp = fuzz.model[split]
        assert _per(per) == wp and _table(blocks) == wb and rows == wr
    assert len(fuzz.model[50][0]) > len(fuzz.model[0][0]) == len(fuzz.items)
    assert b"N" in fuzz.model[0][1]
    # split 0: the rows give back P, T and the runs (the pairs are aligned: = stands over equal bytes, X over different ones)
    blocks, rows, _ = gpu.maf_rows(fuzz.S, fuzz.S.results, fuzz.words, 0)
    for b, (P, T, runs) in zip(_table(blocks), fuzz.cases):
        off, cols = b[0], b[6]
        p2, t2, r2 = MM.undo(rows[off:off + cols], rows[off + cols:off + 2 * cols], b[7])
        assert (p2, t2, r2) == (P, T, runs)


def test_fuzz_by_reference_into_a_seqstore(gpu, fuzz):
    """the same problems as windows of one stored sequence (every third text as the reverse complement of its stored bases)"""
    store = gpu.seqstore()
    try:
        blob, refs = bytearray(), []
        for i, it in enumerate(fuzz.items):
            P, T = it[0], it[1]
            rev = i % 3 == 0
            po = len(blob)
            blob += P
            to = len(blob)
            blob += T[::-1].translate(RC) if rev else T
            refs.append(dict(pattern_seq=0, pattern_off=po, plen=len(P), text_seq=0, text_off=to, tlen=len(T), text_revcomp=1 if rev else 0, mode=UNI))
        assert store.add(bytes(blob)) == 0
        S = gpu.upload_refs(store, refs)
        try:
            for split in (0, 50):
                blocks, rows, per = gpu.maf_rows(S, fuzz.S.results, fuzz.words, split)
                wb, wr, wp = fuzz.model[split]
                assert _per(per) == wp and _table(blocks) == wb and rows == wr
        finally:
            S.free()
    finally:
        store.free()


# ---- 7. the align driver ----
def _align(handles, case, out, maf, split=0, left=False, **params):
    capi.set_maf(maf, split)
    capi.set_left_align(left)
    try:
        if len(handles) == 1:
            summ = capi.align_paf(handles[0], case.fa, case.paf, out, params=params or None)
        else:
            summ = capi.align_paf_multi(handles, case.fa, case.paf, out, params=params or None)
        return open(out, "rb").read(), (open(maf, "rb").read() if maf else None), capi.maf_counts(), summ
    finally:
        capi.set_maf(None)
        capi.set_left_align(False)


def _records_of(paf_lines):
    """the PAF's own records as maf_model.maf_text takes them"""
    out = []
    for line in paf_lines:
        f = line.rstrip("\n").split("\t")
        out.append(dict(qname=f[0], qsize=int(f[1]), qs=int(f[2]), qe=int(f[3]), strand=f[4], tname=f[5], tsize=int(f[6]), ts=int(f[7]), te=int(f[8]),
                        runs=M.parse([v for v in f[12:] if v.startswith("cg:Z:")][0][5:])))
    return out


def _counts_of(text, n_records):
    blocks = MM.parse_maf(text)
    return (n_records, len(blocks), sum(len(b["row_p"]) for b in blocks), 0)


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows, the aligned PAF of a run without the switch and the MAF file of one with it: made once, never changed"""
    d = str(tmp_path_factory.mktemp("maf"))
    fa, paf, seqs = LT._make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, seqs=seqs)
    c.text, none, counts, _ = _align([gpu], c, os.path.join(d, "plain.paf"), None)
    assert none is None and counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20 and any(l.split("\t")[4] == "-" for l in c.lines)
    c.with_text, c.maf, c.counts, _ = _align([gpu], c, os.path.join(d, "with.paf"), os.path.join(d, "with.maf"))
    return c


def test_driver_plain(gpu, case):
    assert case.with_text == case.text  # not one PAF byte changes
    want = MM.maf_text(_records_of(case.lines), case.seqs)  # from the written lines and the FASTA alone
    assert case.maf == want and case.counts == _counts_of(want, len(case.lines))
    blocks = MM.parse_maf(case.maf)
    assert len(blocks) == len(case.lines) and {b["qstrand"] for b in blocks} == {"+", "-"}
    # every block gives back its line's CIGAR
    for b, r in zip(blocks, _records_of(case.lines)):
        assert MM.undo(b["row_p"], b["row_t"], b["score"])[2] == r["runs"]
    # the switch off again: the bytes of the run without it, no counts
    again, none, counts, _ = _align([gpu], case, os.path.join(case.dir, "off.paf"), None)
    assert again == case.text and none is None and counts == (0, 0, 0, 0)


def test_driver_split(gpu, case):
    text, maf, counts, _ = _align([gpu], case, os.path.join(case.dir, "s.paf"), os.path.join(case.dir, "s.maf"), split=4)
    want = MM.maf_text(_records_of(case.lines), case.seqs, 4)
    assert text == case.text and maf == want and counts == _counts_of(want, len(case.lines))
    assert counts[1] > case.counts[1] and counts[2] < case.counts[2]
    # breaks drop gap columns only: the aligned columns are those of the one-block file
    aligned = lambda t: sum(sum(a != 45 and b != 45 for a, b in zip(k["row_p"], k["row_t"])) for k in MM.parse_maf(t))
    assert aligned(maf) == aligned(case.maf)


def test_driver_with_left_align(gpu, case):
    plain, _, _, _ = _align([gpu], case, os.path.join(case.dir, "la0.paf"), None, left=True)
    text, maf, counts, _ = _align([gpu], case, os.path.join(case.dir, "la.paf"), os.path.join(case.dir, "la.maf"), left=True)
    assert text == plain != case.text
    want = MM.maf_text(_records_of(text.decode().splitlines()), case.seqs)
    assert maf == want and counts == _counts_of(want, len(case.lines))
    assert maf != case.maf  # the rows are those of the normalised CIGAR


def test_driver_with_resident_sequences(gpu, case):
    plain, _, _, s0 = _align([gpu], case, os.path.join(case.dir, "r0.paf"), None, resident_sequences=1)
    text, maf, counts, s1 = _align([gpu], case, os.path.join(case.dir, "r1.paf"), os.path.join(case.dir, "r1.maf"), resident_sequences=1)
    assert plain == text == case.text and maf == case.maf and counts == case.counts
    assert s1.records_resident == s0.records_resident > 0 and s1.lazy_fetches <= s0.lazy_fetches  # the host needs no record's bases for the rows


def test_driver_two_handles_on_one_device(gpu, case):
    h2 = capi.Handle(0)
    try:
        text, maf, counts, _ = _align([gpu, h2], case, os.path.join(case.dir, "m.paf"), os.path.join(case.dir, "m.maf"))
    finally:
        h2.close()
    assert text == case.text and maf == case.maf and counts == case.counts


def test_driver_sam(gpu, case):
    """the file does not depend on the main format"""
    plain, _, _, _ = _align([gpu], case, os.path.join(case.dir, "p.sam"), None, sam_format=1)
    text, maf, counts, _ = _align([gpu], case, os.path.join(case.dir, "w.sam"), os.path.join(case.dir, "sam.maf"), sam_format=1)
    assert text == plain and text != case.text and maf == case.maf and counts == case.counts


def test_maf_paf_entry_point(gpu, case):
    out = os.path.join(case.dir, "offline.maf")
    counts = capi.maf_paf(gpu, case.fa, os.path.join(case.dir, "plain.paf"), out)
    assert open(out, "rb").read() == case.maf and counts == case.counts
    counts = capi.maf_paf(gpu, case.fa, os.path.join(case.dir, "plain.paf"), out, split=4)
    want = MM.maf_text(_records_of(case.lines), case.seqs, 4)
    assert open(out, "rb").read() == want and counts == _counts_of(want, len(case.lines))


def test_maf_paf_skips_and_counts(gpu, case, capfd):
    """lines the entry point cannot spell are skipped and counted, each under its own reason, and the others are written as before: one
    without an =XID cg:Z:, one malformed, one whose query neither file has, one whose tlen is not the file's"""
    f = case.lines[3].split("\t")
    bad = ["\t".join(x for x in f if not x.startswith("cg:Z:")) + "\tcg:Z:%dM" % (int(f[8]) - int(f[7])),
           "\t".join(f[:11]),
           "\t".join(["no#such#seq"] + f[1:]),
           "\t".join(f[:6] + [str(int(f[6]) + 1)] + f[7:])]
    paf, out = os.path.join(case.dir, "mixed.paf"), os.path.join(case.dir, "mixed.maf")
    lines = list(case.lines)
    for k, b in enumerate(bad):
        lines.insert(2 + 5 * k, b)
    with open(paf, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    capfd.readouterr()
    counts = capi.maf_paf(gpu, case.fa, paf, out)
    err = capfd.readouterr().err
    assert open(out, "rb").read() == case.maf and counts == case.counts
    assert ("[wfmash::maf] %d records, %d blocks, %d columns, 0 records left without blocks, 4 lines skipped (1 without an =XID cg:Z:, 1 malformed, "
            "1 with an unknown sequence, 1 with another length)" % case.counts[:3]) in err


# ---- 8. the command line on LPA ----
def _cli(args, cwd=None):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "300", CLI] + args, capture_output=True, text=True, cwd=cwd)


@pytest.fixture(scope="module")
def lpa(tmp_path_factory):
    """the sequences, the all-vs-all mapping (as test_cs_gpu maps it) and its alignment with --maf: made once"""
    d = tmp_path_factory.mktemp("maf_lpa")
    seqs, name = {}, None
    for line in gzip.open(LPA, "rt"):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.strip())
    seqs = {k: "".join(v).encode() for k, v in seqs.items()}
    m, a0, a1, maf = str(d / "map.paf"), str(d / "plain.paf"), str(d / "with.paf"), str(d / "out.maf")
    for args in (["-m", "-p", "90", "-P", "50k", "-t", "8", "--out", m, LPA], ["-i", m, "-t", "8", "--out", a0, LPA]):
        r = _cli(args, cwd=str(d))
        assert r.returncode == 0, r.stderr[-500:]
    r = _cli(["--maf", maf, "-i", m, "-t", "8", "--out", a1, LPA], cwd=str(d))
    assert r.returncode == 0, r.stderr[-500:]
    lines = open(a0).read().splitlines()
    assert len(lines) >= 100 and open(a1).read().splitlines() == lines
    return types.SimpleNamespace(dir=d, seqs=seqs, map=m, lines=lines, maf=open(maf, "rb").read(), stderr=r.stderr)


def _summary(stderr):
    m = re.search(r"\[wfmash::maf\] (\d+) records, (\d+) blocks, (\d+) columns, (\d+) records left without blocks", stderr)
    assert m, stderr[-500:]
    return tuple(int(x) for x in m.groups())


def test_cli_lpa(lpa):
    records = _records_of(lpa.lines)
    assert lpa.maf == MM.maf_text(records, lpa.seqs)
    blocks = MM.parse_maf(lpa.maf)
    assert len(blocks) == len(records)
    eq = x = 0
    for b, r in zip(blocks, records):
        _, _, runs = MM.undo(b["row_p"], b["row_t"], b["score"])
        assert runs == r["runs"]  # every line's CIGAR, from the file
        eq += sum(n for n, op in runs if op == "M")
        x += sum(n for n, op in runs if op == "X")
    # the "aligned bases" of the file are the PAF's own = and X totals
    assert eq == sum(n for r in records for n, op in r["runs"] if op == "M") and x == sum(n for r in records for n, op in r["runs"] if op == "X")
    assert _summary(lpa.stderr) == (len(records), len(blocks), sum(len(b["row_p"]) for b in blocks), 0)


def test_cli_lpa_split(lpa):
    out, maf = str(lpa.dir / "split.paf"), str(lpa.dir / "split.maf")
    r = _cli(["--maf", maf, "--maf-split", "50", "-i", lpa.map, "-t", "8", "--out", out, LPA], cwd=str(lpa.dir))
    assert r.returncode == 0, r.stderr[-500:]
    assert open(out).read().splitlines() == lpa.lines
    text = open(maf, "rb").read()
    records = _records_of(lpa.lines)
    assert text == MM.maf_text(records, lpa.seqs, 50)
    blocks, one = MM.parse_maf(text), MM.parse_maf(lpa.maf)
    aligned = lambda bl: sum(sum(a != 45 and b != 45 for a, b in zip(k["row_p"], k["row_t"])) for k in bl)
    assert len(blocks) > len(one) and aligned(blocks) == aligned(one)  # more blocks, the same aligned columns: breaks drop gap columns only
    assert _summary(r.stderr) == (len(records), len(blocks), sum(len(b["row_p"]) for b in blocks), 0)
