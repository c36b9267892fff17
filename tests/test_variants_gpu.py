"""--variants on the device: wfm_call_variants on hand-built problems, at the edges of the write kernel's slices and of both kernels' run
staging, on odd layouts, in chunks and on aligned pairs against the grammar's model (tests/variants_model.py), field by field and allele
byte by allele byte; then the align driver and the command line."""
import ctypes as C
import os
import random
import re
import subprocess
import types

import numpy as np
import pytest

from tests import left_align_model as M
from tests import test_left_align_gpu as LT  # its synthetic pangenome and line helpers (nothing of it is collected from here)
from tests import variants_model as V
from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
RC = bytes.maketrans(b"ACGT", b"TGCA")
UNI = capi.WFM_MODE_END2END_UNI
SLICE = capi.WFM_VAR_SLICE
SNV, INS, DEL, MASKED = V.SNV, V.INS, V.DEL, V.MASKED


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
    """(P, T, runs) of a CIGAR over seeded random bases (the records are called from the runs: the bases need not fit them)"""
    runs = M.parse(cigar)
    P = synth.random_dna(seed, sum(n for n, o in runs if o != "I"))
    T = synth.random_dna(seed + 1000, sum(n for n, o in runs if o != "D"))
    return P, T, runs


def _valid_case(cigar, seed=1):
    """(P, T, runs) where T is what the CIGAR makes of a random P: M over equal bases, X over different ones"""
    runs = M.parse(cigar)
    P = synth.random_dna(seed, sum(n for n, o in runs if o != "I"))
    ins = synth.random_dna(seed + 1000, sum(n for n, o in runs if o == "I") + 1)
    T, p, i = bytearray(), 0, 0
    for n, op in runs:
        if op == "M":
            T += P[p:p + n]
        elif op == "X":
            T += P[p:p + n].translate(RC)
        elif op == "I":
            T += ins[i:i + n]
            i += n
        p += n if op != "I" else 0
    return P, bytes(T), runs


def _call(gpu, cases):
    items, results, words = _pack(cases)
    S = gpu.upload(items)
    try:
        return gpu.call_variants(S, results, words)
    finally:
        S.free()


def _records_of(got, i):
    """problem i's records as [V.Rec], with the fields the model does not carry checked on the way"""
    recs, blob, per = got
    out = []
    for k in range(per[i].first, per[i].first + per[i].count):
        r = recs[k]
        assert r["problem"] == i
        off = int(r["off"])
        out.append(V.Rec(int(r["kind"]), int(r["p"]), int(r["t"]), blob[off:off + r["ref_len"]], blob[off + r["ref_len"]:off + r["ref_len"] + r["alt_len"]]))
    return out


def _assert_model(got, cases, names=None):
    recs, blob, per = got
    first, off = 0, 0
    for i, (P, T, runs) in enumerate(cases):
        name = names[i] if names else i
        want, ends = V.variants_of(P, T, runs)
        assert (per[i].flags, per[i].n_runs, per[i].end_gaps) == (0, len(runs), ends), name
        assert (per[i].first, per[i].count) == (first, len(want)), name
        mine = recs[first:first + len(want)]
        assert (mine["problem"] == i).all(), name
        assert mine["kind"].tolist() == [r.kind for r in want], name
        assert mine["p"].tolist() == [r.p for r in want] and mine["t"].tolist() == [r.t for r in want], name
        assert mine["ref_len"].tolist() == [len(r.ref) for r in want] and mine["alt_len"].tolist() == [len(r.alt) for r in want], name
        alleles = b"".join(r.ref + r.alt for r in want)
        sizes = np.array([len(r.ref) + len(r.alt) for r in want], dtype=np.int64)
        assert mine["off"].tolist() == (off + np.concatenate(([0], np.cumsum(sizes)[:-1]))).tolist() if len(want) else True, name
        assert blob[off:off + len(alleles)] == alleles, name
        first += len(want)
        off += len(alleles)
    assert len(recs) == first and len(blob) == off


def _assert_inverse(got, cases):
    """apply(P, records) == T, for cases whose CIGAR is valid and has no end gaps"""
    for i, (P, T, _) in enumerate(cases):
        assert V.apply(P, _records_of(got, i)) == T, i


# ---- 1. hand cases, the expected records written out ----
R = V.Rec
HAND = [
    # name, P, T, CIGAR, records, end gaps
    ("some_before", b"ACGTA", b"ACCTA", "2=1X2=", [R(SNV, 2, 2, b"G", b"C")], 0),
    ("m_only", b"ACGTA", b"ACGTA", "5=", [], 0),
    ("some_behind", b"ACGTA", b"AGTA", "1=1D3=", [R(DEL, 0, 1, b"AC", b"A")], 0),
    ("x_only_with_n", b"ACT", b"GTN", "3X", [R(SNV, 0, 0, b"A", b"G"), R(SNV, 1, 1, b"C", b"T"), R(SNV | MASKED, 2, 2, b"T", b"N")], 0),
    ("lower_case_is_not_masked", b"aC-", b"Gt*", "3X", [R(SNV, 0, 0, b"a", b"G"), R(SNV, 1, 1, b"C", b"t"), R(SNV | MASKED, 2, 2, b"-", b"*")], 0),
    ("end_gaps_are_counted", b"ACTCC", b"GGACT", "2I3=2D", [], 2),
    ("ins_then_del_share_an_anchor", b"ACGTAGGGTTCCA", b"ACGTACCTTCCA", "5=2I3D5=",
     [R(INS, 4, 5, b"A", b"ACC"), R(DEL, 4, 7, b"AGGG", b"A")], 0),
    ("del_then_ins_share_no_base", b"ACGTAGGGTTCCA", b"ACGTACCTTCCA", "5=3D2I5=",
     [R(DEL, 4, 5, b"AGGG", b"A"), R(INS, 7, 5, b"G", b"GCC")], 0),
    ("gap_behind_an_x", b"ACGTCGA", b"ACGATTCGA", "3=1X2I3=", [R(SNV, 3, 3, b"T", b"A"), R(INS, 3, 4, b"T", b"TTT")], 0),
    ("anchor_is_the_first_base", b"ACGT", b"AGGCGT", "1=2I3=", [R(INS, 0, 1, b"A", b"AGG")], 0),
    ("no_anchor_behind_a_leading_ins", b"ACGT", b"TTGT", "2I2D2=", [], 2),
]


def test_hand_cases_record_for_record(gpu):
    cases = [(P, T, M.parse(cg)) for _, P, T, cg, _, _ in HAND]
    got = _call(gpu, cases)
    for i, (name, _, _, _, want, ends) in enumerate(HAND):
        assert _records_of(got, i) == want, name
        assert got[2][i].end_gaps == ends, name
    _assert_model(got, cases, [h[0] for h in HAND])
    # every one of them without end gaps is a valid CIGAR
    for i, (name, P, T, _, _, ends) in enumerate(HAND):
        if ends == 0:
            assert V.apply(P, _records_of(got, i)) == T, name


# ---- 2. the edges of a slice ----
NEIGHBOUR = (b"ACGTA", b"ACCTA", [(2, "M"), (1, "X"), (2, "M")])  # behind every case: an overrun shows in it


def _edge_cases():
    c = {}
    for d in (-1, 0, 1):  # a deletion of L bases has L + 2 allele bytes
        c["alleles_of_slice%+d" % d] = "5=%dD5=" % (SLICE + d - 2)
    c["snv_ref_closes_a_slice_alt_opens_the_next"] = "5=%dD3=1X5=" % (SLICE - 3)  # the SNV's REF is byte SLICE - 1
    c["snv_opens_a_slice"] = "5=%dD3=1X5=" % (SLICE - 2)
    c["ins_anchor_closes_a_slice"] = "5=%dD3=7I5=" % (SLICE - 3)   # REF | anchor + 7 bases
    c["ins_alt_anchor_opens_a_slice"] = "5=%dD3=7I5=" % (SLICE - 4)
    c["record_in_slice_0_bytes_through_slice_4"] = "5=70000D5="
    c["ins_of_70000"] = "5=70000I5="
    c["del_record_in_slice_k_bytes_through_k_plus_2"] = "5=%dX3=40000D5=" % (SLICE // 2 + 100)
    c["x_run_of_20000_across_slices"] = "3=20000X3="
    return c


def test_slice_edges(gpu):
    edge = _edge_cases()
    names, cases = [], []
    for k, (name, cg) in enumerate(edge.items()):
        names += [name, name + ":neighbour"]
        cases += [_valid_case(cg, seed=0xE0 + k), NEIGHBOUR]
    got = _call(gpu, cases)
    _assert_model(got, cases, names)
    _assert_inverse(got, cases)


def test_slice_edges_each_first_in_the_output(gpu):
    """the same problems where the slices are counted from their own first byte, and the cases are what their names say"""
    for k, (name, cg) in enumerate(_edge_cases().items()):
        cases = [_valid_case(cg, seed=0xE0 + k), NEIGHBOUR]
        got = _call(gpu, cases)
        _assert_model(got, cases, [name, name + ":neighbour"])
        recs, blob, per = got
        mine = recs[:per[0].count]
        total = int((mine["ref_len"] + mine["alt_len"]).sum())
        for d in (-1, 0, 1):
            if name == "alleles_of_slice%+d" % d:
                assert total == SLICE + d
        if name == "snv_ref_closes_a_slice_alt_opens_the_next":
            assert (mine[1]["kind"], mine[1]["off"]) == (SNV, SLICE - 1)
        if name == "ins_anchor_closes_a_slice":
            assert (mine[1]["kind"], mine[1]["off"]) == (INS, SLICE - 1)
        if name in ("record_in_slice_0_bytes_through_slice_4", "ins_of_70000"):
            assert mine[0]["off"] == 0 and total == 70002 > 4 * SLICE
        if name == "del_record_in_slice_k_bytes_through_k_plus_2":
            first, last = int(mine[-1]["off"]) // SLICE, (int(mine[-1]["off"]) + 40001) // SLICE
            assert mine[-1]["kind"] == DEL and first == 1 and last >= first + 2


# ---- 3. run counts at the edges of the kernels' staging ----
CYCLE = ("3=", "1X", "2=", "2I", "1=", "1D", "4=", "2X")


def _cigar_of_runs(n):
    return "".join(CYCLE[i % len(CYCLE)] for i in range(n))


@pytest.mark.parametrize("counts", [(255, 256, 257), (1023, 1024, 1025)], ids=["index_carry", "write_staging"])
def test_run_count_edges(gpu, counts):
    names, cases = [], []
    for n in counts:
        names += ["%d_runs" % n, "%d_runs:neighbour" % n]
        cases += [_valid_case(_cigar_of_runs(n), seed=0xA0 + n), NEIGHBOUR]
    got = _call(gpu, cases)
    _assert_model(got, cases, names)
    for i, (P, T, runs) in enumerate(cases):
        assert got[2][i].n_runs == len(runs) and runs[-1][1] in "MX"
    _assert_inverse(got, cases)


def test_twenty_thousand_runs(gpu):
    cases = [_valid_case("1=1X" * 10000, seed=0xA7), NEIGHBOUR]
    got = _call(gpu, cases)
    _assert_model(got, cases)
    _assert_inverse(got, cases)
    assert got[2][0].count == 10000


# ---- 4. layout and flags ----
def test_reverse_order_with_unused_words(gpu):
    cases = [(P, T, M.parse(cg)) for _, P, T, cg, _, _ in HAND] + [_case("30=2X1I400=7D3=", seed=3)]
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
        got = gpu.call_variants(S, results, np.array(words, dtype=np.uint32))
    finally:
        S.free()
    _assert_model(got, cases)


def test_not_done_spans_and_bad_arguments(gpu):
    P, T, runs = _case("20=1X3I30=2D10=", seed=5)
    w = M.to_words(runs)
    n_ops = sum(n for n, _ in runs)
    short = M.to_words([(runs[0][0] - 1, "M")] + runs[1:])               # one base short of plen
    zero = M.to_words(runs[:2] + [(0, "I")] + runs[3:])                  # a run of length 0
    twice = M.to_words([(10, "M"), (10, "M")] + runs[1:])                # two neighbours of one op
    blocks = [w, short, w, zero, w, twice, w]
    offs = np.cumsum([0] + [len(b) for b in blocks]).tolist()
    words = np.array(sum(blocks, []), dtype=np.uint32)
    # (-300: WFM_ST_UNREACHABLE)
    items = [(P, T, UNI | capi.WFM_MODE_SCORE_ONLY), (P, T, UNI), (b"", b"", UNI)] + [(P, T, UNI)] * 7
    results = [(0, 27, 0, 0, 0), (-300, -1, 0, n_ops, len(w)), (0, 0, 0, 0, 0)] + [(0, -1, offs[k], n_ops, len(blocks[k])) for k in range(7)]
    want, _ = V.variants_of(P, T, runs)
    nbytes = sum(len(r.ref) + len(r.alt) for r in want)
    S = gpu.upload(items)
    try:
        got = gpu.call_variants(S, results, words)
        recs, blob, per = got
        ND, SP = capi.WFM_VAR_NOT_DONE, capi.WFM_VAR_SPANS
        assert [c.flags for c in per] == [ND, ND, ND, 0, SP, 0, SP, 0, SP, 0]
        assert [c.count for c in per] == [0, 0, 0, len(want), 0, len(want), 0, len(want), 0, len(want)]
        assert [c.first for c in per] == [0, 0, 0, 0] + [len(want) * k for k in (1, 1, 2, 2, 3, 3)]
        for i in (3, 5, 7, 9):  # the neighbours of the flagged problems untouched
            assert _records_of(got, i) == want
        assert len(recs) == 4 * len(want) and len(blob) == 4 * nbytes
        # the return value: the number of problems flagged WFM_VAR_SPANS
        arr = (capi.Result * len(results))()
        for i, (status, score, ops_off, ops_len, n_runs) in enumerate(results):
            arr[i].status, arr[i].score, arr[i].ops_off, arr[i].ops_len, arr[i].n_runs = status, score, ops_off, ops_len, n_runs
        vp, ap, nv, nb, pr = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0), (capi.VarCall * len(results))()
        rc = gpu._L.wfm_call_variants(gpu._p, S._p, arr, words.ctypes.data, len(words), C.byref(vp), C.byref(nv), C.byref(ap), C.byref(nb), pr)
        assert rc == 3 and (nv.value, nb.value) == (4 * len(want), 4 * nbytes)
        gpu._L.wfm_free_variants(vp, ap)
        # a run range past the buffer: WFM_E_ARG, and the handle goes on working
        bad = list(results)
        bad[9] = (0, -1, offs[6] + 1, n_ops, len(w))
        with pytest.raises(capi.WfmError, match=r"\(-3\).*leave the run buffer"):
            gpu.call_variants(S, bad, words)
        again = gpu.call_variants(S, results, words)
        assert again[0].tobytes() == recs.tobytes() and again[1] == blob
    finally:
        S.free()


def test_no_problems(gpu):
    S = gpu.upload([])
    try:
        recs, blob, per = gpu.call_variants(S, [], np.zeros(0, dtype=np.uint32))
        assert (len(recs), blob, per) == (0, b"", [])
    finally:
        S.free()


# ---- 5. chunks ----
def test_chunks_of_one_mib_and_two_calls(gpu, monkeypatch):
    """three problems of about 1.1 MB of alleles each (a chunk of its own each: one alone exceeds the block) with small ones between, which
    share chunks"""
    cases = []
    for k in range(3):
        cases.append(_valid_case("5=%dD3=20000X2=%dI5=" % (500000 + 1000 * k, 550000 - 3000 * k), seed=0xC40 + k))
        cases += [NEIGHBOUR, _valid_case("40=3I20=2X9=4D30=", seed=0xC50 + k)]
    items, results, words = _pack(cases)
    S = gpu.upload(items)
    try:
        default = gpu.call_variants(S, results, words)
        monkeypatch.setenv("WFM_VAR_OUT_MB", "1")
        small = gpu.call_variants(S, results, words)
        twice = gpu.call_variants(S, results, words)
    finally:
        S.free()
    assert 3200000 < len(default[1]) < 3400000
    _assert_model(default, cases)
    for other in (small, twice):
        assert other[0].tobytes() == default[0].tobytes() and other[1] == default[1]
        assert [(c.flags, c.first, c.count, c.end_gaps) for c in other[2]] == [(c.flags, c.first, c.count, c.end_gaps) for c in default[2]]


# ---- 6. aligned pairs ----
def _without_end_gaps(P, T, runs):
    """what applying the records makes of P where the first or last runs are gaps the call leaves alone: the pattern's bases under a
    D stay, the text's under an I never come"""
    lead_i = lead_d = trail_i = trail_d = 0
    if runs[0][1] in "ID":
        if runs[0][1] == "I":
            lead_i = runs[0][0]
            if len(runs) > 2 and runs[1][1] == "D":  # no pattern base before it
                lead_d = runs[1][0]
        else:
            lead_d = runs[0][0]
    if len(runs) > 1 and runs[-1][1] in "ID":
        if runs[-1][1] == "I":
            trail_i = runs[-1][0]
        else:
            trail_d = runs[-1][0]
    return P[:lead_d] + T[lead_i:len(T) - trail_i] + P[len(P) - trail_d:]


@pytest.fixture(scope="module")
def pairs(gpu):
    """36 pairs of 2 to 20 kb at 1 to 10 % divergence, aligned once: seqset, results, runs; never changed"""
    rng = random.Random(0x7A1)
    items = []
    for i in range(36):
        P = synth.random_dna(0x7A100 + i, rng.randint(2000, 20000) if i % 6 else 2000 + 3000 * (i // 6))
        T = synth.mutate(P, (0.01, 0.03, 0.1)[i % 3], 0x7A200 + i)
        items.append((P, T, UNI))
    S = gpu.upload(items)
    failed, words = gpu.align_resident_rle(S)
    assert failed == 0
    yield types.SimpleNamespace(items=items, S=S, words=words)
    S.free()


def _pairs_check(got, items, results, words):
    cases = [(it[0], it[1], M.from_words(words[results[i].ops_off:results[i].ops_off + results[i].n_runs])) for i, it in enumerate(items)]
    _assert_model(got, cases)
    for i, (P, T, runs) in enumerate(cases):
        assert V.apply(P, _records_of(got, i)) == _without_end_gaps(P, T, runs), i
    return cases


def test_aligned_pairs_equal_the_model_and_invert(gpu, pairs):
    got = gpu.call_variants(pairs.S, pairs.S.results, pairs.words)
    cases = _pairs_check(got, pairs.items, pairs.S.results, pairs.words)
    kinds = got[0]["kind"] & 255
    assert (kinds == SNV).sum() > 1000 and (kinds == INS).sum() > 100 and (kinds == DEL).sum() > 100
    assert sum(1 for P, T, runs in cases if runs[0][1] in "MX" and runs[-1][1] in "MX") >= 30  # mostly T itself


def test_aligned_pairs_left_aligned(gpu, pairs):
    res, words, stats = gpu.left_align(pairs.S, pairs.S.results, pairs.words)
    assert all(s.flags == 0 for s in stats) and sum(s.moved for s in stats) > 0
    got = gpu.call_variants(pairs.S, res, words)
    cases = _pairs_check(got, pairs.items, res, words)
    # every INS and DEL is at its leftmost rotation: nothing the rule could still move
    for P, T, runs in cases:
        assert M.movable(P, T, runs) == []


# ---- 7. the align driver and the command line ----
def _align(gpu, case, out, vcf, left=False, cs=0, **params):
    capi.set_variants(vcf)
    capi.set_left_align(left)
    capi.set_cs(cs)
    try:
        capi.align_paf(gpu, case.fa, case.paf, out, params=params or None)
        return open(out, "rb").read(), (open(vcf).read().splitlines() if vcf else None), capi.variants_counts()
    finally:
        capi.set_variants(None)
        capi.set_left_align(False)
        capi.set_cs(0)


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows, the aligned PAF of a run without the switch and the VCF of one with it: made once, never changed"""
    d = str(tmp_path_factory.mktemp("variants"))
    fa, paf, seqs = LT._make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, seqs=seqs)
    c.text, none, counts = _align(gpu, c, os.path.join(d, "plain.paf"), None)
    assert none is None and counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20 and any(l.split("\t")[4] == "-" for l in c.lines) and any(l.split("\t")[4] == "+" for l in c.lines)
    c.vcf_path = os.path.join(d, "plain.vcf")
    c.with_text, c.vcf, c.counts = _align(gpu, c, os.path.join(d, "with.paf"), c.vcf_path)
    return c


def _body(vcf):
    return [l for l in vcf if not l.startswith("#")]


def _lines_of_paf(paf_lines, seqs, records_of):
    """the VCF lines the PAF lines imply; records_of(fields, cigar, P, T) -> [V.Rec]"""
    out, masked = [], 0
    for line in paf_lines:
        f, cg = LT._split(line)
        P, T = LT._bases(seqs, f)
        recs = records_of(f, cg, P, T)
        masked += sum(1 for r in recs if r.kind & MASKED)
        out += V.vcf_lines(recs, f[5], int(f[7]), f[0], int(f[2]), int(f[3]), f[4])
    return out, masked


def _from_cigar(f, cg, P, T):
    recs, ends = V.variants_of(P, T, M.parse(cg))
    assert ends == 0  # a line's CIGAR has no end gaps
    assert V.apply(P, recs) == T
    return recs


def test_driver_leaves_the_paf_alone_and_writes_the_header(gpu, case):
    assert case.with_text == case.text
    head = [l for l in case.vcf if l.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.2" and re.fullmatch(r"##source=wfmash-hip \S+", head[1])
    version = head[1].split(" ", 1)[1]
    assert head == V.header(version, [(name, len(s)) for name, s in case.seqs.items()])
    assert case.vcf[:len(head)] == head  # nothing but records behind it
    records, written, masked, alone = case.counts
    assert (records, written, alone) == (len(case.lines), len(_body(case.vcf)), 0) and written > 100


def test_driver_lines_are_the_cigars(gpu, case):
    want, masked = _lines_of_paf(case.lines, case.seqs, _from_cigar)
    assert _body(case.vcf) == want and case.counts[2] == masked


def test_driver_lines_against_the_fastas(gpu, case):
    """REF is the target at POS; the query at [QSTART, QEND), reverse-complemented on '-', is ALT without its anchor; ascending POS within
    a record"""
    strands = set()
    for l in _body(case.vcf):
        chrom, pos, _, ref, alt, _, _, info = l.split("\t")
        kv = dict(x.split("=") for x in info.split(";"))
        pos, a, b = int(pos), int(kv["QSTART"]), int(kv["QEND"])
        assert case.seqs[chrom][pos - 1:pos - 1 + len(ref)] == ref.encode()
        q = case.seqs[kv["QNAME"]][a:b]
        if kv["QSTRAND"] == "-":
            q = q[::-1].translate(RC)
        snv = len(ref) == 1 and len(alt) == 1
        assert q == (alt if snv else alt[1:]).encode() and (snv or ref[0] == alt[0])
        strands.add(kv["QSTRAND"])
    assert strands == {"+", "-"}
    # within a record POS ascends: hold the file against the PAF lines' own sorted lists
    want, _ = _lines_of_paf(case.lines, case.seqs, _from_cigar)
    at = 0
    for line in case.lines:
        f, cg = LT._split(line)
        P, T = LT._bases(case.seqs, f)
        n = sum(1 for r in V.variants_of(P, T, M.parse(cg))[0] if not r.kind & MASKED)
        pos = [int(l.split("\t")[1]) for l in want[at:at + n]]
        assert pos == sorted(pos)
        at += n
    assert at == len(want)


def test_driver_with_cs_equals_the_cs_strings(gpu, case):
    text, vcf, counts = _align(gpu, case, os.path.join(case.dir, "cs.paf"), os.path.join(case.dir, "cs.vcf"), cs=1)
    lines = text.decode().splitlines()
    assert [l.rpartition("\tcs:Z:")[0] for l in lines] == case.lines

    def from_cs(f, cg, P, T):
        cs = [x for x in f if x.startswith("cs:Z:")][0][5:].encode()
        return V.from_cs(cs, P)

    want, _ = _lines_of_paf(lines, case.seqs, from_cs)
    assert _body(vcf) == want and vcf == case.vcf
    assert counts == case.counts


def test_driver_with_left_align(gpu, case):
    text, vcf, counts = _align(gpu, case, os.path.join(case.dir, "la.paf"), os.path.join(case.dir, "la.vcf"), left=True)
    assert text != case.text  # the pangenome plants gaps in repeats
    want, _ = _lines_of_paf(text.decode().splitlines(), case.seqs, _from_cigar)
    assert _body(vcf) == want and vcf != case.vcf
    assert (counts[0], counts[1], counts[3]) == (len(case.lines), len(want), 0)
    # all three switches: one upload serves them, and the lines are the same
    text3, vcf3, _ = _align(gpu, case, os.path.join(case.dir, "la3.paf"), os.path.join(case.dir, "la3.vcf"), left=True, cs=2)
    assert vcf3 == vcf and [l.rpartition("\tcs:Z:")[0] for l in text3.decode().splitlines()] == text.decode().splitlines()


def test_driver_with_resident_sequences(gpu, case):
    text, vcf, counts = _align(gpu, case, os.path.join(case.dir, "r.paf"), os.path.join(case.dir, "r.vcf"), resident_sequences=1)
    assert text == case.text and vcf == case.vcf and counts == case.counts


def _cli(args, cwd=None):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "120", CLI] + args, capture_output=True, text=True, cwd=cwd)


def test_cli_writes_the_same_file_and_its_counts(case):
    out, vcf = os.path.join(case.dir, "cli.paf"), os.path.join(case.dir, "cli.vcf")
    r = _cli(["--variants", vcf, "--gpus", "1", "--resident-seqs", "-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert open(out, "rb").read() == case.text and open(vcf).read().splitlines() == case.vcf
    m = re.search(r"\[wfmash::variants\] (\d+) records, (\d+) variants written, (\d+) SNVs masked, (\d+) records left alone", r.stderr)
    assert m and tuple(int(x) for x in m.groups()) == case.counts
