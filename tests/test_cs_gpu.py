"""--cs on the device: wfm_cs_strings on hand-built problems, at the edges of the write kernel's slices, on odd layouts and on aligned
pairs against the grammar's model (tests/cs_model.py); then the align driver and the command line with the switch off, short and long."""
import ctypes as C
import gzip
import os
import random
import re
import subprocess
import types

import numpy as np
import pytest

from oracle import wflign_host as W
from tests import cs_model as CS
from tests import left_align_model as M
from tests import test_left_align_gpu as LT  # its synthetic pangenome and line helpers (nothing of it is collected from here)
from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
LPA = os.path.join(ROOT, "tests", "golden", "LPA.subset.fa.gz")
RC = bytes.maketrans(b"ACGT", b"TGCA")
UNI = capi.WFM_MODE_END2END_UNI
SLICE = capi.WFM_CS_SLICE
FORMS = (CS.SHORT, CS.LONG)


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
    """(P, T, runs) of a CIGAR over seeded random bases (the string is spelled from the runs: the bases need not fit them)"""
    runs = M.parse(cigar)
    P = synth.random_dna(seed, sum(n for n, o in runs if o != "I"))
    T = synth.random_dna(seed + 1000, sum(n for n, o in runs if o != "D"))
    return P, T, runs


def _spell_all(gpu, cases):
    """both forms of every case: {form: ([bytes], [Cs])}, one upload"""
    items, results, words = _pack(cases)
    S = gpu.upload(items)
    try:
        return {form: gpu.cs_strings(S, results, words, form) for form in FORMS}
    finally:
        S.free()


def _assert_model(got, cases, names=None):
    for form in FORMS:
        strings, per = got[form]
        off = 0
        for i, (P, T, runs) in enumerate(cases):
            want = CS.cs_of(P, T, runs, form)
            name = (names[i] if names else i, form)
            assert per[i].flags == 0 and per[i].n_runs == len(runs), name
            assert (per[i].off, per[i].len) == (off, len(want)), name
            assert strings[i] == want, name
            off += len(want)


# ---- 1. hand cases ----
HAND = [
    # name, P, T, CIGAR, short, long
    ("m_only", b"ACGTA", b"ACGTA", "5=", b":5", b"=ACGTA"),
    ("x_only_with_n", b"ACT", b"GTN", "3X", b"*ag*ct*tn", b"*ag*ct*tn"),
    ("i_only", b"", b"ACGN", "4I", b"+acgn", b"+acgn"),
    ("d_only", b"TTGA", b"", "4D", b"-ttga", b"-ttga"),
    ("i_first_d_last", b"ACTCC", b"GGACT", "2I3=2D", b"+gg:3-cc", b"+gg=ACT-cc"),
    ("d_first_i_last", b"CCACT", b"ACTGG", "2D3=2I", b"-cc:3+gg", b"-cc=ACT+gg"),
    ("x_first_x_last", b"AACTGG", b"CACTTT", "1X3=2X", b"*ac:3*gt*gt", b"*ac=ACT*gt*gt"),
    ("m_first_m_last", b"ACGT", b"ACNGT", "2=1I2=", b":2+n:2", b"=AC+n=GT"),
    ("lower_case_stays", b"AcgT", b"TcgA", "1X2=1X", b"*at:2*ta", b"*at=cg*ta"),
    ("x_over_equal_m_over_different", b"AAGG", b"AATT", "2X2=", b"*aa*aa:2", b"*aa*aa=GG"),
    ("other_bytes_stay", b"A-*", b"A", "1=2D", b":1--*", b"=A--*"),
]
DIGITS = (1, 9, 10, 99, 100, 65535, 65536, 1000000)


def test_hand_cases_byte_for_byte(gpu):
    cases = [(P, T, M.parse(cg)) for _, P, T, cg, _, _ in HAND]
    got = _spell_all(gpu, cases)
    for i, (name, _, _, _, short, long_) in enumerate(HAND):
        assert got[CS.SHORT][0][i] == short, name
        assert got[CS.LONG][0][i] == long_, name
    _assert_model(got, cases, [h[0] for h in HAND])


def test_m_runs_of_every_digit_count(gpu):
    """1 .. 7 digits each as a problem of its own, then all of them in one problem between X runs"""
    cases = []
    for k, L in enumerate(DIGITS):
        P = synth.random_dna(0xD1 + k, L)
        cases.append((P, P, [(L, "M")]))
    cases.append(_case("1X".join("%d=" % L for L in DIGITS), seed=0xD9))
    got = _spell_all(gpu, cases)
    for k, L in enumerate(DIGITS):
        assert got[CS.SHORT][0][k] == b":%d" % L
        assert got[CS.LONG][0][k] == b"=" + cases[k][0]
    _assert_model(got, cases)


# ---- 2. the edges of a slice ----
NEIGHBOUR = (b"ACG", b"ACG", [(3, "M")])  # behind every case: an overrun shows in it


def _edge_cases():
    c = {}
    for d in (-1, 0, 1):  # the long form spells 1 + L bytes of an M run of L
        c["long_string_of_slice%+d" % d] = "%d=" % (SLICE + d - 1)
    for d in (-1, 0, 1):  # the short form: ':1' + '-' + L bases
        c["short_string_of_slice%+d" % d] = "1=%dD" % (SLICE + d - 3)
    for k in range(3):    # long form: the X triple begins at byte 1 + L; byte k of it is the next slice's first
        c["long_x_triple_byte%d_opens_a_slice" % k] = "%d=2X5=" % (SLICE - 1 - k)
    for k in range(3):    # short form: ':1' + '-' + L bases, then the triple
        c["short_x_triple_byte%d_opens_a_slice" % k] = "1=%dD2X5=" % (SLICE - 3 - k)
    c["short_inside_a_number"] = "1=%dD123456=" % (SLICE - 7)   # ':123' | '456'
    c["short_behind_a_sign"] = "1=%dD1=3I" % (SLICE - 6)        # ':1' '-' L bases ':1' '+' | 3 bases
    c["long_behind_a_sign"] = "%d=3I2=" % (SLICE - 2)           # '=' L bases '+' | 3 bases
    c["d_of_70000"] = "5=70000D5="
    c["m_of_70000"] = "3I70000=2X"
    c["20000_runs"] = "1=1X" * 10000
    return c


def test_slice_edges(gpu):
    edge = _edge_cases()
    names, cases = [], []
    for k, (name, cg) in enumerate(edge.items()):
        names += [name, name + ":neighbour"]
        cases += [_case(cg, seed=0xE0 + k), NEIGHBOUR]
    got = _spell_all(gpu, cases)
    _assert_model(got, cases, names)
    # the cases are what their names say
    by = {n: i for i, n in enumerate(names)}
    for d in (-1, 0, 1):
        assert got[CS.LONG][1][by["long_string_of_slice%+d" % d]].len == SLICE + d
        assert got[CS.SHORT][1][by["short_string_of_slice%+d" % d]].len == SLICE + d
    for k in range(3):
        i = by["long_x_triple_byte%d_opens_a_slice" % k]
        assert got[CS.LONG][0][i][SLICE - k] == ord("*")
        assert got[CS.SHORT][0][by["short_x_triple_byte%d_opens_a_slice" % k]][SLICE - k] == ord("*")
    assert got[CS.SHORT][0][by["short_inside_a_number"]][SLICE - 4:SLICE + 3] == b":123456"
    assert got[CS.SHORT][0][by["short_behind_a_sign"]][SLICE - 1] == ord("+")
    assert got[CS.LONG][0][by["long_behind_a_sign"]][SLICE - 1] == ord("+")


def test_slice_edges_each_first_in_the_output(gpu):
    """the same strings where the slices are counted from their own first byte (in test_slice_edges every case lies behind the ones
    before it, at whatever offset they leave)"""
    for k, (name, cg) in enumerate(_edge_cases().items()):
        cases = [_case(cg, seed=0xE0 + k), NEIGHBOUR]
        _assert_model(_spell_all(gpu, cases), cases, [name, name + ":neighbour"])


# ---- 3. layout ----
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
        got = {form: gpu.cs_strings(S, results, np.array(words, dtype=np.uint32), form) for form in FORMS}
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
        for form in FORMS:
            want = CS.cs_of(P, T, runs, form)
            f = gpu._L.wfm_cs_strings
            strings, per = gpu.cs_strings(S, results, words, form)
            assert [c.flags for c in per] == [capi.WFM_CS_NOT_DONE] * 3 + [0, capi.WFM_CS_SPANS, 0]
            assert [c.len for c in per] == [0, 0, 0, len(want), 0, len(want)]
            assert [c.off for c in per] == [0, 0, 0, 0, len(want), len(want)]
            assert strings == [b"", b"", b"", want, b"", want]  # the neighbours of the flagged problem untouched
            # the return value: the number of problems flagged WFM_CS_SPANS
            arr = (capi.Result * len(results))()
            for i, (status, score, ops_off, ops_len, n_runs) in enumerate(results):
                arr[i].status, arr[i].score, arr[i].ops_off, arr[i].ops_len, arr[i].n_runs = status, score, ops_off, ops_len, n_runs
            out_p, total, pr = C.c_void_p(), C.c_size_t(0), (capi.Cs * len(results))()
            rc = f(gpu._p, S._p, arr, words.ctypes.data, len(words), form, C.byref(out_p), C.byref(total), pr)
            assert rc == 1 and total.value == 2 * len(want)
            gpu._L.wfm_free_cs(out_p)
            # a run range past the buffer: WFM_E_ARG, and the handle goes on working
            bad = list(results)
            bad[5] = (0, -1, 2 * len(w) + 1, n_ops, len(w))
            with pytest.raises(capi.WfmError, match=r"\(-3\).*leave the run buffer"):
                gpu.cs_strings(S, bad, words, form)
            again, _ = gpu.cs_strings(S, results, words, form)
            assert again == strings
        with pytest.raises(capi.WfmError, match=r"\(-3\).*form 2"):
            gpu.cs_strings(S, results, words, 2)
        assert gpu.cs_strings(S, results, words, CS.SHORT)[0][3] == CS.cs_of(P, T, runs, CS.SHORT)
    finally:
        S.free()


def test_no_problems(gpu):
    S = gpu.upload([])
    try:
        assert gpu.cs_strings(S, [], np.zeros(0, dtype=np.uint32), CS.LONG) == ([], [])
    finally:
        S.free()


def test_output_in_chunks_of_one_mib(gpu, monkeypatch):
    """about 3 MB of long-form output through a 1 MiB output block: problems of 200 kB to 400 kB in chunks of several, one of
    1.2 MB in a chunk of its own"""
    rng = random.Random(0xC4)
    cases = []
    for k, L in enumerate((200000, 400000, 300000, 1200000, 300000, 350000, 200000)):
        parts, left = [], L
        while left > 0:
            m = min(left, rng.randint(1, 40000))
            parts.append("%d=" % m)
            left -= m
            if left > 0:
                parts.append(rng.choice(["1X", "2X", "3I", "40D", "1I", "1D"]))
        cases.append(_case("".join(parts), seed=0xC40 + k))
    items, results, words = _pack(cases)
    S = gpu.upload(items)
    try:
        default = gpu.cs_strings(S, results, words, CS.LONG)[0]
        monkeypatch.setenv("WFM_CS_OUT_MB", "1")
        small = gpu.cs_strings(S, results, words, CS.LONG)[0]
        small_short = gpu.cs_strings(S, results, words, CS.SHORT)[0]
    finally:
        S.free()
    assert 2900000 < sum(len(s) for s in default) < 3200000
    assert small == default
    for (P, T, runs), s, sh in zip(cases, default, small_short):
        assert s == CS.cs_of(P, T, runs, CS.LONG) and sh == CS.cs_of(P, T, runs, CS.SHORT)


def test_output_of_several_host_copies(gpu):
    """9.3 MB of long-form output in one chunk: it comes down in pieces of 4 MiB, two full ones and a rest, and a problem lies across
    each of the two seams"""
    cases = [_case("%d=1X%d=3I%d=" % (L, L // 2, L // 3), seed=0xB16 + k) for k, L in enumerate((1500000, 1700000, 1900000))]
    got = _spell_all(gpu, cases)
    assert 2 * (4 << 20) < sum(len(s) for s in got[CS.LONG][0]) < 3 * (4 << 20)
    _assert_model(got, cases)


# ---- 4. fuzz: aligned pairs ----
def _fuzz_items():
    rng = random.Random(0xC5A1)
    items = []
    for i in range(256):
        P, T, _ = M.mutated_pair(rng, rng.randint(200, 3000), (0.02, 0.08, 0.2)[i % 3])
        if i in (7, 130):  # an N in both: the byte kernels align it, and the string carries it as n
            k = len(P) // 3
            P = P[:k] + b"N" * 12 + P[k + 12:]
            T = T[:k // 2] + b"NNN" + T[k // 2 + 3:]
        items.append((P, T, UNI) if i % 8 == 5 else (P, T))
    return items


@pytest.fixture(scope="module")
def fuzz(gpu):
    """the pairs, aligned once: seqset, results and runs, and the model's strings in both forms; never changed"""
    items = _fuzz_items()
    S = gpu.upload(items)
    failed, words = gpu.align_resident_rle(S)
    assert failed == 0
    runs = [M.from_words(words[S.results[i].ops_off:S.results[i].ops_off + S.results[i].n_runs]) for i in range(S.n)]
    model = {form: [CS.cs_of(it[0], it[1], r, form) for it, r in zip(items, runs)] for form in FORMS}
    yield types.SimpleNamespace(items=items, S=S, words=words, runs=runs, model=model)
    S.free()


def test_fuzz_equals_the_model_and_decodes(gpu, fuzz):
    for form in FORMS:
        strings, per = gpu.cs_strings(fuzz.S, fuzz.S.results, fuzz.words, form)
        assert all(c.flags == 0 for c in per)
        assert strings == fuzz.model[form]
        for (P, T), s in zip((it[:2] for it in fuzz.items), strings):
            if form == CS.LONG:
                p2, t2 = CS.decode(s)
                assert CS.same_bases(p2, P) and CS.same_bases(t2, T)
            else:
                assert CS.same_bases(CS.decode(s, P), T)
    assert sum(len(s) for s in fuzz.model[CS.SHORT]) > 50000
    assert b"n" in fuzz.model[CS.SHORT][7] + fuzz.model[CS.LONG][7]


def test_fuzz_through_align_rle(gpu, fuzz):
    """the runs as align_rle returns them (a list per problem), packed again with unused words between the problems"""
    sub = fuzz.items[:24]
    res = gpu.align_rle(sub)
    cases = []
    for it, (r, _) in zip(sub, res):
        cases.append((it[0], it[1], [(int(n), op if isinstance(op, str) else chr(op) if isinstance(op, int) else op.decode()) for n, op in r.ops]))
    _assert_model(_spell_all(gpu, cases), cases)


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
            for form in FORMS:
                strings, per = gpu.cs_strings(S, fuzz.S.results, fuzz.words, form)
                assert all(c.flags == 0 for c in per) and strings == fuzz.model[form]
        finally:
            S.free()
    finally:
        store.free()


# ---- 5. the align driver ----
def _align(gpu, case, out, form, left=False, **params):
    capi.set_cs(form)
    capi.set_left_align(left)
    try:
        summ = capi.align_paf(gpu, case.fa, case.paf, out, params=params or None)
        return open(out, "rb").read(), capi.cs_counts(), summ
    finally:
        capi.set_cs(0)
        capi.set_left_align(False)


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows and the aligned PAF of a run without the switch: made once, never changed"""
    d = str(tmp_path_factory.mktemp("cs"))
    fa, paf, seqs = LT._make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, seqs=seqs)
    c.text, counts, c.summ = _align(gpu, c, os.path.join(d, "plain.paf"), 0)
    assert counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20 and all("cg:Z:" in l and "cs:Z:" not in l for l in c.lines)
    assert any(l.split("\t")[4] == "-" for l in c.lines)
    return c


def _check_lines(plain_lines, text, seqs, form):
    """every line is the plain line + one last field, and that field is the model's string of the line's CIGAR over the bases its
    coordinates name (the reverse complement of query [qs, qe) for a '-' line), which it decodes back to; returns the strings' bytes"""
    lines = text.decode().splitlines()
    assert len(lines) == len(plain_lines)
    total = 0
    for old, new in zip(plain_lines, lines):
        head, _, cs = new.rpartition("\tcs:Z:")
        assert head == old
        f, cg = LT._split(old)
        P, T = LT._bases(seqs, f)
        cs = cs.encode()
        assert cs == CS.cs_of(P, T, M.parse(cg), CS.LONG if form == 2 else CS.SHORT)
        if form == 2:
            p2, t2 = CS.decode(cs)
            assert CS.same_bases(p2, P) and CS.same_bases(t2, T)
        else:
            assert CS.same_bases(CS.decode(cs, P), T)
        total += len(cs)
    return total


@pytest.mark.parametrize("form", [1, 2], ids=["short", "long"])
def test_driver_appends_only_the_field(gpu, case, form):
    text, (records, nbytes, without, zero), _ = _align(gpu, case, os.path.join(case.dir, "cs%d.paf" % form), form)
    assert _check_lines(case.lines, text, case.seqs, form) == nbytes
    assert (records, without, zero) == (len(case.lines), 0, 0)
    # the verifier reads such a file as it reads the plain one
    checked, failed, unverifiable, _ = capi.verify_paf(gpu, case.fa, os.path.join(case.dir, "cs%d.paf" % form))
    assert (checked, failed, unverifiable) == (len(case.lines), 0, 0)
    # off again: the bytes of the run without the switch, and no counts
    again, counts, _ = _align(gpu, case, os.path.join(case.dir, "off.paf"), 0)
    assert again == case.text and counts == (0, 0, 0, 0)


@pytest.mark.parametrize("form", [1, 2], ids=["short", "long"])
def test_driver_with_left_align(gpu, case, form):
    la, _, _ = _align(gpu, case, os.path.join(case.dir, "la.paf"), 0, left=True)
    assert la != case.text  # the pangenome plants gaps in repeats
    text, (records, nbytes, without, _), _ = _align(gpu, case, os.path.join(case.dir, "la_cs%d.paf" % form), form, left=True)
    assert _check_lines(la.decode().splitlines(), text, case.seqs, form) == nbytes
    assert (records, without) == (len(case.lines), 0)


@pytest.mark.parametrize("form", [1, 2], ids=["short", "long"])
def test_driver_with_resident_sequences(gpu, case, form):
    plain, _, s0 = _align(gpu, case, os.path.join(case.dir, "r0.paf"), 0, resident_sequences=1)
    assert plain == case.text
    text, (records, _, without, _), s1 = _align(gpu, case, os.path.join(case.dir, "r%d.paf" % form), form, resident_sequences=1)
    eager, _, _ = _align(gpu, case, os.path.join(case.dir, "e%d.paf" % form), form)
    assert text == eager
    assert (records, without) == (len(case.lines), 0)
    assert s1.records_resident == s0.records_resident > 0 and s1.lazy_fetches <= s0.lazy_fetches  # the host needs no record's bases for the string


# ---- 6. the command line on LPA ----
def _cli(args, cwd=None):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "300", CLI] + args, capture_output=True, text=True, cwd=cwd)


@pytest.fixture(scope="module")
def lpa(tmp_path_factory):
    """the sequences, the all-vs-all mapping and its alignment without the flag: made once"""
    d = tmp_path_factory.mktemp("cs_lpa")
    seqs, name = {}, None
    for line in gzip.open(LPA, "rt"):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.strip())
    seqs = {k: "".join(v).encode() for k, v in seqs.items()}
    m, a0 = str(d / "map.paf"), str(d / "plain.paf")
    for args in (["-m", "-p", "90", "-P", "50k", "-t", "8", "--out", m, LPA], ["-i", m, "-t", "8", "--out", a0, LPA]):
        r = _cli(args, cwd=str(d))
        assert r.returncode == 0, r.stderr[-500:]
    lines = open(a0).read().splitlines()
    assert len(lines) >= 100
    return types.SimpleNamespace(dir=d, seqs=seqs, map=m, lines=lines)


@pytest.mark.parametrize("flag,form", [("--cs", 1), ("--cs=short", 1), ("--cs=long", 2)], ids=["bare", "short", "long"])
def test_cli_lpa_paf(lpa, flag, form):
    out = str(lpa.dir / ("cs_%s.paf" % flag.strip("-").replace("=", "_")))
    r = _cli([flag, "-i", lpa.map, "-t", "8", "--out", out, LPA], cwd=str(lpa.dir))
    assert r.returncode == 0, r.stderr[-500:]
    nbytes = _check_lines(lpa.lines, open(out, "rb").read(), lpa.seqs, form)
    m = re.search(r"\[wfmash::cs\] (\d+) records, (\d+) bytes \((short|long)\), 0 records left without a string", r.stderr)
    assert m and (int(m.group(1)), int(m.group(2)), m.group(3)) == (len(lpa.lines), nbytes, "long" if form == 2 else "short")


def test_cli_lpa_sam(lpa):
    plain, out = str(lpa.dir / "plain.sam"), str(lpa.dir / "cs.sam")
    for args in (["-a", "-i", lpa.map, "-t", "8", "--out", plain, LPA], ["-a", "--cs", "-i", lpa.map, "-t", "8", "--out", out, LPA]):
        r = _cli(args, cwd=str(lpa.dir))
        assert r.returncode == 0, r.stderr[-500:]
    old, new = open(plain).read().splitlines(), open(out).read().splitlines()
    assert len(old) == len(new)
    records = 0
    for x, y in zip(old, new):
        if x.startswith("@"):
            assert x == y
            continue
        head, _, cs = y.rpartition("\tcs:Z:")
        assert head == x
        f = x.split("\t")
        runs = M.parse(f[5])
        start = int(f[3]) - 1
        P = W.upper_valid_dna(lpa.seqs[f[2]][start:start + sum(n for n, o in runs if o != "I")])
        assert f[9] != "*" and CS.decode(cs.encode(), P).upper() == f[9].encode()
        assert cs.encode() == CS.cs_of(P, f[9].encode(), runs, CS.SHORT)
        records += 1
    assert records == len(lpa.lines)
