"""--left-align on the device: wfm_left_align_runs on hand-built problems and on aligned repeat-rich pairs against the rule's model
(tests/left_align_model.py), then the align driver and the command line with the switch on and off, and the LPA all-vs-all run."""
import gzip
import os
import random
import re
import subprocess
import types

import numpy as np
import pytest

from oracle import wflign_host as W
from tests import left_align_cases as LC
from tests import left_align_model as M
from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
LPA = os.path.join(ROOT, "tests", "golden", "LPA.subset.fa.gz")
RC = bytes.maketrans(b"ACGT", b"TGCA")
UNI = capi.WFM_MODE_END2END_UNI


def _pack(cases):
    """[(P, T, runs)] -> (items for upload, results as tuples, the runs of all problems as words)"""
    items, results, words = [], [], []
    for P, T, runs in cases:
        items.append((P, T, UNI))
        w = M.to_words(runs)
        results.append((0, -1, len(words), sum(n for n, _ in runs), len(w)))
        words += w
    return items, results, np.array(words, dtype=np.uint32)


def _runs_of(res, words, i):
    return M.from_words(words[res[i].ops_off:res[i].ops_off + res[i].n_runs])


# ---- 1. hand-built problems ----
def test_hand_cases_run_for_run(gpu):
    cases = [(P, T, M.parse(cg)) for _, P, T, cg, _ in LC.HAND]
    items, results, words = _pack(cases)
    S = gpu.upload(items)
    try:
        res, out, stats = gpu.left_align(S, results, words)
    finally:
        S.free()
    for i, (name, P, T, cg, want) in enumerate(LC.HAND):
        got = _runs_of(res, out, i)
        model, shifts = M.left_align(P, T, M.parse(cg))
        assert M.spell(got) == want, name
        assert got == model, name
        s = stats[i]
        assert s.flags == 0 and s.runs_out == len(got), name
        assert (s.gaps, s.moved, s.bases_moved, s.longest) == (len(shifts), sum(1 for d in shifts if d), sum(shifts), max(shifts + [0])), name
        assert res[i].ops_len == results[i][3] and res[i].score == -1
    # the run count: one fewer where the M run is used up against an X, one more where an X follows the gap
    by_name = {c[0]: i for i, c in enumerate(LC.HAND)}
    assert stats[by_name["m_consumed"]].runs_out == 4 and stats[by_name["x_follows"]].runs_out == 5
    assert sum(int(r.n_runs) for r in res) == len(out)


@pytest.mark.parametrize("name,P,T,cigar,want", LC.LONG, ids=[c[0] for c in LC.LONG])
def test_long_homopolymer_crosses_both_paths(gpu, name, P, T, cigar, want):
    """70 000 bases: past the lane path's threshold, through the wave path's 1024-byte steps, to index 1 or 0 of the sequence"""
    items, results, words = _pack([(P, T, M.parse(cigar))])
    S = gpu.upload(items)
    try:
        res, out, stats = gpu.left_align(S, results, words)
        assert M.spell(_runs_of(res, out, 0)) == want
        assert stats[0].flags == 0 and stats[0].moved == 1 and stats[0].longest == stats[0].bases_moved == M.parse(want)[2][0] - 10
        flagged, ck = gpu.check_runs(S, res, out)
        assert flagged == 0 and ck[0].flags == 0
    finally:
        S.free()


def test_not_done_spans_and_bad_range(gpu):
    name, P, T, cg, want = LC.HAND[0]
    runs = M.parse(cg)
    w = M.to_words(runs)
    short = M.to_words([(runs[0][0] - 1, "M")] + runs[1:])  # one base short of plen
    items = [(P, T, UNI | capi.WFM_MODE_SCORE_ONLY), (P, T, UNI), (P, T, UNI), (P, T, UNI)]
    words = np.array(w + short + w, dtype=np.uint32)
    n_ops = sum(n for n, _ in runs)
    # (-300: WFM_ST_UNREACHABLE)
    results = [(0, 27, 0, 0, 0), (-300, -1, 0, n_ops, len(w)), (0, -1, len(w), n_ops - 1, len(short)), (0, -1, 2 * len(w), n_ops, len(w))]
    S = gpu.upload(items)
    try:
        res, out, stats = gpu.left_align(S, results, words)
        assert [s.flags for s in stats] == [capi.WFM_LA_NOT_DONE, capi.WFM_LA_NOT_DONE, capi.WFM_LA_SPANS, 0]
        assert res[0].n_runs == 0 and res[0].score == 27
        assert list(out[res[1].ops_off:res[1].ops_off + res[1].n_runs]) == w           # verbatim
        assert list(out[res[2].ops_off:res[2].ops_off + res[2].n_runs]) == short       # verbatim
        assert M.spell(_runs_of(res, out, 3)) == want
        assert all(s.moved == 0 and s.gaps == 0 for s in stats[:3])
        # a run range past the buffer: WFM_E_ARG, and the handle goes on working
        bad = list(results)
        bad[3] = (0, -1, 2 * len(w) + 1, n_ops, len(w))
        with pytest.raises(capi.WfmError, match=r"\(-3\).*leave the run buffer"):
            gpu.left_align(S, bad, words)
        res2, out2, _ = gpu.left_align(S, results, words)
        assert list(out2) == list(out)
    finally:
        S.free()


# ---- 2. fuzz: aligned repeat-rich pairs ----
def _fuzz_items():
    rng = random.Random(0xA11C)
    items = []
    for i in range(256):
        P, T, _ = M.mutated_pair(rng, rng.randint(200, 3000), (0.02, 0.08, 0.2)[i % 3])
        if i in (7, 130):  # an N in both: the byte kernels align it, bytes are compared as bytes
            k = len(P) // 3
            P = P[:k] + b"N" * 12 + P[k + 12:]
            T = T[:k // 2] + b"NNN" + T[k // 2 + 3:]
        if i % 8 == 3:
            items.append((P, T, capi.WFM_MODE_ENDSFREE, 20, 15, 10, 25))
        elif i % 8 == 5:
            items.append((P, T, UNI))
        else:
            items.append((P, T))
    return items


@pytest.fixture(scope="module")
def fuzz(gpu):
    """the pairs, aligned once: seqset, results and runs before, and the model's answer per problem; never changed"""
    items = _fuzz_items()
    S = gpu.upload(items)
    failed, words = gpu.align_resident_rle(S)
    assert failed == 0
    before = [_runs_of(S.results, words, i) for i in range(S.n)]
    model = [M.left_align(it[0], it[1], r) for it, r in zip(items, before)]
    yield types.SimpleNamespace(items=items, S=S, words=words, before=before, model=model)
    S.free()


def test_fuzz_equals_the_model(gpu, fuzz):
    res, out, stats = gpu.left_align(fuzz.S, fuzz.S.results, fuzz.words)
    n_gaps = n_moved = 0
    for i, (want, shifts) in enumerate(fuzz.model):
        assert _runs_of(res, out, i) == want, i
        s = stats[i]
        assert s.flags == 0, i  # the inputs give the model neither a span error nor a problem without runs
        assert (s.gaps, s.moved, s.bases_moved) == (len(shifts), sum(1 for d in shifts if d), sum(shifts)), i
        n_gaps += s.gaps
        n_moved += s.moved
    assert n_gaps > 5000 and n_moved > 500
    # valid, with the price and the counts it had
    _, ck0 = gpu.check_runs(fuzz.S, fuzz.S.results, fuzz.words)
    flagged, ck1 = gpu.check_runs(fuzz.S, res, out)
    assert flagged == 0
    fields = ("score", "matches", "mismatches", "ins_runs", "ins_bases", "del_runs", "del_bases")
    for i, (a, b) in enumerate(zip(ck0, ck1)):
        assert a.flags == b.flags == 0, i
        assert [getattr(a, f) for f in fields] == [getattr(b, f) for f in fields], i
        assert b.score == fuzz.S.results[i].score == res[i].score
    # a second application changes nothing
    res2, out2, stats2 = gpu.left_align(fuzz.S, res, out)
    assert list(out2) == list(out) and all(s.moved == 0 for s in stats2)
    assert [(r.ops_off, r.n_runs) for r in res2] == [(r.ops_off, r.n_runs) for r in res]


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
            r = dict(pattern_seq=0, pattern_off=po, plen=len(P), text_seq=0, text_off=to, tlen=len(T), text_revcomp=1 if rev else 0, mode=UNI)
            refs.append(r)
        assert store.add(bytes(blob)) == 0
        S = gpu.upload_refs(store, refs)
        try:
            res, out, stats = gpu.left_align(S, fuzz.S.results, fuzz.words)
        finally:
            S.free()
        for i, (want, _) in enumerate(fuzz.model):
            assert stats[i].flags == 0 and _runs_of(res, out, i) == want, i
    finally:
        store.free()


# ---- 3. the align driver ----
def _write_fasta(path, seqs, width=70):
    with open(path, "w") as f:
        for name, s in seqs.items():
            f.write(">" + name + "\n")
            s = s.decode()
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + "\n")


def _make_case(d, seed=0x1EF7A, n_hap=4, L=40000, rows=24):
    """4 haplotypes of 40 kb and a reverse-complemented one, 24 mapping rows; every 2 kb a (CA)n or an An tract whose length differs
    between the haplotypes, so that gaps in repeats do not depend on chance"""
    rng = random.Random(seed)
    base = bytearray(synth.random_dna(seed, L))
    sites = list(range(1000, L - 1000, 2000))
    seqs = {}

    def with_tracts(h):
        out, at = bytearray(), 0
        for k, pos in enumerate(sites):
            out += base[at:pos]
            out += b"CA" * (40 - 2 * ((h + k) % 3)) if k % 2 == 0 else b"A" * (60 - 3 * ((h + 2 * k) % 4))
            at = pos
        return bytes(out + base[at:])

    for h in range(n_hap):
        seqs["hap%d#1#chr1" % h] = synth.mutate(with_tracts(h), rng.choice([0.005, 0.01, 0.02]), seed * 100 + h)
    seqs["hap9#1#chr1"] = synth.mutate(with_tracts(9), 0.01, seed * 100 + 9)[::-1].translate(RC)
    fa = os.path.join(d, "pan.fa")
    _write_fasta(fa, seqs)
    names = list(seqs)
    lines = []
    for chain in range(1, rows + 1):
        qn, tn = ("hap9#1#chr1", rng.choice(names[:-1])) if chain % 3 == 0 else rng.sample(names, 2)
        ql, tl = len(seqs[qn]), len(seqs[tn])
        seg = rng.choice([3000, 6000, 9000])
        qs = rng.randrange(0, min(ql, tl) - seg - 600)
        qe = qs + seg
        rev = (qn == "hap9#1#chr1") != (tn == "hap9#1#chr1")
        ts, te = (tl - qe, tl - qs) if rev else (qs, qe)
        ts = max(0, ts + rng.randrange(-60, 60))
        te = min(tl, te + rng.randrange(-60, 60))
        lines.append("\t".join(map(str, [qn, ql, qs, qe, "-" if rev else "+", tn, tl, ts, te, 100, seg, 30, "id:f:0.97", "kc:f:0.9", "ch:Z:%d.1.1" % chain])))
    paf = os.path.join(d, "map.paf")
    with open(paf, "w") as f:
        f.write("\n".join(lines) + "\n")
    return fa, paf, seqs


def _align(gpu, case, out, left, **params):
    capi.set_left_align(left)
    try:
        capi.align_paf(gpu, case.fa, case.paf, out, params=params or None)
        return open(out, "rb").read(), capi.left_align_counts()
    finally:
        capi.set_left_align(False)


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows and the aligned PAF of a run without the switch: made once, never changed"""
    d = str(tmp_path_factory.mktemp("leftalign"))
    fa, paf, seqs = _make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, seqs=seqs, plain=os.path.join(d, "plain.paf"))
    c.text, counts = _align(gpu, c, c.plain, False)
    assert counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20 and all("cg:Z:" in l for l in c.lines)
    return c


def _bases(seqs, f):
    """(P, T) of a PAF line's fields: target [ts, te), query [qs, qe) strand-adjusted, normalised as the driver's windows are"""
    q = W.upper_valid_dna(seqs[f[0]][int(f[2]):int(f[3])])
    if f[4] == "-":
        q = W.revcomp(q)
    return W.upper_valid_dna(seqs[f[5]][int(f[7]):int(f[8])]), q


def _split(line):
    f = line.split("\t")
    cg = [x for x in f if x.startswith("cg:Z:")][0]
    return [x for x in f if x is not cg], cg[5:]


def _compare_with_plain(case, text, seqs=None):
    """same lines, same fields but cg:Z:, every new CIGAR the model's answer for the old one; returns the number of changed lines"""
    seqs = seqs or case.seqs
    lines = text.decode().splitlines()
    assert len(lines) == len(case.lines)
    changed = 0
    for old, new in zip(case.lines, lines):
        f0, cg0 = _split(old)
        f1, cg1 = _split(new)
        assert f0 == f1
        P, T = _bases(seqs, f0)
        want, _ = M.left_align(P, T, M.parse(cg0))
        assert cg1 == M.spell(want)
        assert M.movable(P, T, M.parse(cg1)) == []
        changed += cg0 != cg1
    return changed


def test_driver_left_aligns_only_the_cigars(gpu, case):
    text, (records, gaps, moved, alone) = _align(gpu, case, os.path.join(case.dir, "la.paf"), True)
    assert _compare_with_plain(case, text) >= 1
    assert records >= len(case.lines) and gaps > 0 and moved > 0 and alone == 0
    checked, failed, unverifiable, _ = capi.verify_paf(gpu, case.fa, os.path.join(case.dir, "la.paf"))
    assert (checked, failed, unverifiable) == (len(case.lines), 0, 0)
    # off again: the bytes of the run without the switch, and no counts
    again, counts = _align(gpu, case, os.path.join(case.dir, "off.paf"), False)
    assert again == case.text and counts == (0, 0, 0, 0)


def test_driver_with_resident_sequences(gpu, case):
    plain, counts0 = _align(gpu, case, os.path.join(case.dir, "r0.paf"), False, resident_sequences=1)
    assert plain == case.text and counts0 == (0, 0, 0, 0)
    text, (records, gaps, moved, alone) = _align(gpu, case, os.path.join(case.dir, "r1.paf"), True, resident_sequences=1)
    assert _compare_with_plain(case, text) >= 1 and moved > 0 and alone == 0
    checked, failed, unverifiable, _ = capi.verify_paf(gpu, case.fa, os.path.join(case.dir, "r1.paf"))
    assert (checked, failed, unverifiable) == (len(case.lines), 0, 0)


def test_driver_sam_with_md(gpu, case):
    sam0, _ = _align(gpu, case, os.path.join(case.dir, "s0.sam"), False, sam_format=1, emit_md_tag=1)
    sam1, (_, _, moved, alone) = _align(gpu, case, os.path.join(case.dir, "s1.sam"), True, sam_format=1, emit_md_tag=1)
    a = [l.split("\t") for l in sam0.decode().splitlines() if not l.startswith("@")]
    b = [l.split("\t") for l in sam1.decode().splitlines() if not l.startswith("@")]
    assert len(a) == len(b) >= 20 and moved > 0 and alone == 0
    # the writer's MD (wflign_patch.cpp:2397-2478 as oracle/wflign_host.py restates it): of the record's CIGAR, read from the first base of
    # the record's target window -- the mapping row's padded start -- on
    rows = {}
    for line in open(case.paf):
        row = W.parse_mashmap_row(line, 1000, 1000)
        rows[row["chain_id"]] = row
    changed = 0
    for x, y in zip(a, b):
        md_x, md_y = [v for v in x if v.startswith("MD:Z:")][0], [v for v in y if v.startswith("MD:Z:")][0]
        assert [v for k, v in enumerate(x) if k != 5 and v is not md_x] == [v for k, v in enumerate(y) if k != 5 and v is not md_y]
        if x[5] == y[5]:
            assert md_x == md_y
            continue
        changed += 1
        row = rows[int([v for v in y if v.startswith("ci:i:")][0][5:])]
        target = W.upper_valid_dna(case.seqs[y[2]][row["rStartPos"]:row["rEndPos"]])
        assert md_y == W.md_string(y[5], 0, target)
    assert changed >= 1


def _cli(args):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "120", CLI] + args, capture_output=True, text=True)


def test_cli_left_align_with_verify(case):
    out = os.path.join(case.dir, "cli.paf")
    r = _cli(["--left-align", "--verify", "-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    m = re.search(r"\[wfmash::left-align\] (\d+) records, (\d+) interior gaps, (\d+) moved, 0 records left alone", r.stderr)
    assert m and int(m.group(3)) > 0
    assert "[wfmash::verify] %d lines checked, 0 failed, 0 unverifiable" % len(case.lines) in r.stderr
    assert _compare_with_plain(case, open(out, "rb").read()) >= 1


# ---- 4. LPA all-vs-all ----
def test_lpa_all_vs_all(tmp_path):
    seqs, name = {}, None
    for line in gzip.open(LPA, "rt"):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.strip())
    seqs = {k: "".join(v).encode() for k, v in seqs.items()}
    m, a0, a1 = (str(tmp_path / n) for n in ("map.paf", "plain.paf", "la.paf"))
    subprocess.check_call(["timeout", "-k", "10", "300", CLI, "-m", "-p", "90", "-P", "50k", "-t", "8", "--out", m, LPA], cwd=str(tmp_path))
    subprocess.check_call(["timeout", "-k", "10", "300", CLI, "-i", m, "-t", "8", "--out", a0, LPA], cwd=str(tmp_path))
    subprocess.check_call(["timeout", "-k", "10", "300", CLI, "--left-align", "-i", m, "-t", "8", "--out", a1, LPA], cwd=str(tmp_path))
    r = _cli(["--verify-paf", a1, LPA])
    assert r.returncode == 0 and ", 0 failed, 0 unverifiable" in r.stderr, r.stderr[-500:]
    old, new = open(a0).read().splitlines(), open(a1).read().splitlines()
    assert len(old) == len(new) >= 100
    changed = 0
    for x, y in zip(old, new):
        f0, cg0 = _split(x)
        f1, cg1 = _split(y)
        assert f0 == f1
        P, T = _bases(seqs, f1)
        assert M.movable(P, T, M.parse(cg1)) == []
        changed += cg0 != cg1
    print("LPA: %d of %d lines changed by --left-align" % (changed, len(new)))
    assert changed > 0
