"""wfm_check_runs: every CIGAR run held against the bases it covers, on the device (wfmash_amd/csrc/wfa_check.hip).

Expected values come from _walk(), a pure-Python walk over runs written here by hand for hand-made sequence pairs: it shares no code
with the library, and no case but the positive pass uses aligner output, so every path of the kernels is reached by construction --
slice boundaries (WFM_CHECK_SLICE ops per compare task), every relative alignment of the two byte streams and the edges of the 16-byte
loads, the scan's rounds of 256 runs, the structural flags, empty sides, skipped problems, the ends-free price (endsfree_price of
tests/endsfree_cases.py).  Every comparison is exact."""
import itertools

import numpy as np
import pytest

import endsfree_cases as E
from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

S = capi.CHECK_SLICE
M0, EF, UNI, SO = capi.WFM_MODE_END2END_BIWFA, capi.WFM_MODE_ENDSFREE, capi.WFM_MODE_END2END_UNI, capi.WFM_MODE_SCORE_ONLY
NOT_CHECKED, BAD_RUN, SPANS, M_DIFFERS, X_EQUAL, SCORE, COUNTS = (capi.WFM_CK_NOT_CHECKED, capi.WFM_CK_BAD_RUN, capi.WFM_CK_SPANS,
                                                                  capi.WFM_CK_M_DIFFERS, capi.WFM_CK_X_EQUAL, capi.WFM_CK_SCORE, capi.WFM_CK_COUNTS)
OPS = "MXID"
FIELDS = ("flags", "score", "bad_p", "bad_t", "bad_run", "n_runs", "matches", "mismatches", "ins_runs", "ins_bases", "del_runs", "del_bases")
OTHER = {65: 67, 67: 71, 71: 84, 84: 65}  # a base that differs: A -> C -> G -> T -> A


def _gap(pen, n):
    x, o1, e1, o2, e2 = pen
    return 0 if n <= 0 else min(o1 + e1 * n, o2 + e2 * n)


def _price(runs, mode, free, pen):
    """the price of the runs: end to end, each run on its own; ends-free, endsfree_price on the op string they spell"""
    pen = pen or E.DEFAULT_PEN
    if mode == EF:
        return E.endsfree_price("".join(op * n for n, op in runs).encode(), free, pen)
    return sum(pen[0] * n if op == "X" else _gap(pen, n) if op in "ID" else 0 for n, op in runs)


def _walk(p, t, runs, mode=UNI, free=(0, 0, 0, 0), pen=None, score=None, ops_len=None):
    """what wfm_check_runs must report for runs [(length, op)] over pattern p and text t; score / ops_len: what the result claims
    (None: the truth)"""
    pa, ta = np.frombuffer(p, dtype=np.uint8), np.frombuffer(t, dtype=np.uint8)
    free = E.clamp(free, len(p), len(t)) if mode == EF else (0, 0, 0, 0)
    exp = dict.fromkeys(FIELDS, 0)
    exp["bad_p"] = exp["bad_t"] = -1
    exp["n_runs"] = len(runs)
    bad_runs = [i for i, (n, op) in enumerate(runs) if n == 0 or (i > 0 and runs[i - 1][1] == op)]
    pc = sum(n for n, op in runs if op != "I")
    tc = sum(n for n, op in runs if op != "D")
    oc = sum(n for n, op in runs)
    exp["matches"] = sum(n for n, op in runs if op == "M")
    exp["mismatches"] = sum(n for n, op in runs if op == "X")
    exp["ins_runs"] = sum(1 for n, op in runs if op == "I" and n)
    exp["ins_bases"] = sum(n for n, op in runs if op == "I")
    exp["del_runs"] = sum(1 for n, op in runs if op == "D" and n)
    exp["del_bases"] = sum(n for n, op in runs if op == "D")
    price = _price(runs, mode, free, pen) if not bad_runs else _price(runs, UNI, free, pen)
    exp["score"] = price
    flags = 0
    if bad_runs:
        flags |= BAD_RUN
        exp["bad_run"] = bad_runs[0]
    if pc != len(p) or tc != len(t):
        flags |= SPANS
    if oc != (oc if ops_len is None else ops_len):
        flags |= COUNTS
    if score is not None and score >= 0 and score != price:
        flags |= SCORE
    if pc <= len(p) and tc <= len(t):
        i = j = 0
        for r, (n, op) in enumerate(runs):
            if op in "MX":
                same = pa[i:i + n] == ta[j:j + n]
                off = np.flatnonzero(~same if op == "M" else same)
                if len(off):
                    flags |= M_DIFFERS if op == "M" else X_EQUAL
                    if exp["bad_p"] < 0:
                        exp["bad_p"], exp["bad_t"], exp["bad_run"] = i + int(off[0]), j + int(off[0]), r
                i += n
                j += n
            elif op == "I":
                j += n
            else:
                i += n
    exp["flags"] = flags
    return exp


class Case:
    def __init__(self, name, p, t, runs, mode=UNI, free=(0, 0, 0, 0), score=None, ops_len=None, n_runs=None, status=0, expect=None, pen=None):
        self.name, self.p, self.t, self.runs, self.mode, self.free = name, bytes(p), bytes(t), list(runs), mode, tuple(free)
        self.status = status
        self.read = self.runs if n_runs is None else self.runs[:n_runs]   # the runs the result names
        true_ops = sum(n for n, _ in self.runs)
        self.claim_ops = true_ops if ops_len is None else ops_len
        self.claim_score = _price(self.runs, mode & 0xff, E.clamp(free, len(self.p), len(self.t)), pen) if score is None else score
        self.expect = expect if expect is not None else _walk(self.p, self.t, self.read, mode & 0xff, free, pen, self.claim_score, self.claim_ops)


def _run(gpu, cases, pen=None):
    """one upload and one wfm_check_runs for all cases; returns (flagged, [Check])"""
    items = [(c.p, c.t, c.mode) + c.free for c in cases]
    words, results = [], []
    for c in cases:
        results.append((c.status, c.claim_score, len(words), c.claim_ops, len(c.read)))
        words.extend((n << 2) | OPS.index(op) for n, op in c.runs)   # (all of them: a result that names fewer leaves the rest unread)
    ss = gpu.upload(items)
    try:
        return gpu.check_runs(ss, results, np.array(words, dtype=np.uint32), pen)
    finally:
        ss.free()


def _hold(gpu, cases, pen=None):
    flagged, got = _run(gpu, cases, pen)
    for c, g in zip(cases, got):
        have = {f: getattr(g, f) for f in FIELDS}
        assert have == c.expect, (c.name, {f: (have[f], c.expect[f]) for f in FIELDS if have[f] != c.expect[f]})
    assert flagged == sum(1 for c in cases if c.expect["flags"] & ~NOT_CHECKED)
    return got


def _wrong(seq, *at):
    b = bytearray(seq)
    for i in at:
        b[i] = OTHER[b[i]]
    return bytes(b)


def _spell(runs, seed):
    """a pattern and a text that the runs describe exactly: M bases equal, X bases different"""
    p, t = bytearray(), bytearray()
    for k, (n, op) in enumerate(runs):
        s = synth.random_dna(seed * 1000 + k, n)
        if op == "M":
            p += s; t += s
        elif op == "X":
            p += s; t += bytes(OTHER[b] for b in s)
        elif op == "I":
            t += s
        else:
            p += s
    return bytes(p), bytes(t)


def test_slices(gpu):
    """a single M run around the slice length; one wrong base at index 0, at the last index, at the last base of slice 0 and at the
    first base of slice 1: exactly that base is reported"""
    cases = []
    for L in (S - 1, S, S + 1, 2 * S + 5):
        p = synth.random_dna(0xC0 + L, L)
        cases.append(Case("clean%d" % L, p, p, [(L, "M")]))
        for at in sorted({0, L - 1, S - 1, S} & set(range(L))):
            c = Case("L%d_at%d" % (L, at), p, _wrong(p, at), [(L, "M")])
            assert (c.expect["flags"], c.expect["bad_p"], c.expect["bad_t"], c.expect["bad_run"]) == (M_DIFFERS, at, at, 0)
            cases.append(c)
    _hold(gpu, cases)


def test_first_offender(gpu):
    """two wrong bases in different slices: the one with the smaller pattern index is reported, whichever task finishes first"""
    L = 2 * S + 5
    p = synth.random_dna(0xF0, L)
    cases = []
    for a, b in ((5, S + 7), (S - 1, S), (S + 3, 2 * S + 1), (0, L - 1)):
        c = Case("at%d_%d" % (a, b), p, _wrong(p, a, b), [(L, "M")])
        assert c.expect["bad_p"] == a
        cases.append(c)
    # ... and with the runs before them shifting the text: D 3, then M
    c = Case("shifted", synth.random_dna(0xF1, 3) + p, _wrong(p, 2 * S, S + 1), [(3, "D"), (L, "M")])
    assert (c.expect["bad_p"], c.expect["bad_t"], c.expect["bad_run"]) == (S + 4, S + 1, 1)
    cases.append(c)
    _hold(gpu, cases)


def test_relative_alignment(gpu):
    """a leading I or D run of 0 .. 16 bases before an M run of 200 with a wrong base at M offsets 0, 15, 16, 17, 199: every relative
    alignment of the two byte streams, and the edges of the 16-byte loads"""
    body = synth.random_dna(0xA1, 200)
    cases = []
    for op, k in itertools.product("ID", range(17)):
        junk = synth.random_dna(0xA2 + k, k)
        runs = ([(k, op)] if k else []) + [(200, "M")]
        for off in (None, 0, 15, 16, 17, 199):
            other = body if off is None else _wrong(body, off)
            p, t = (body, junk + other) if op == "I" else (junk + body, other)
            c = Case("%s%d_off%s" % (op, k, off), p, t, runs)
            if off is None:
                assert c.expect["flags"] == 0
            else:
                want = (off, k + off) if op == "I" else (k + off, off)
                assert (c.expect["flags"], c.expect["bad_p"], c.expect["bad_t"], c.expect["bad_run"]) == (M_DIFFERS,) + want + (1 if k else 0,)
            cases.append(c)
    _hold(gpu, cases)


def test_x_runs(gpu):
    """an X run of 1, 2 and 17 bases whose k-th base is equal: X_EQUAL at that base; the clean M runs beside it give no flag"""
    cases = []
    for n in (1, 2, 17):
        runs = [(20, "M"), (n, "X"), (23, "M")]
        p, t = _spell(runs, 0x70 + n)
        cases.append(Case("x%d_clean" % n, p, t, runs))
        assert cases[-1].expect["flags"] == 0
        for k in range(n):
            tk = bytearray(t)
            tk[20 + k] = p[20 + k]
            c = Case("x%d_eq%d" % (n, k), p, bytes(tk), runs)
            assert (c.expect["flags"], c.expect["bad_p"], c.expect["bad_t"], c.expect["bad_run"]) == (X_EQUAL, 20 + k, 20 + k, 1)
            cases.append(c)
    _hold(gpu, cases)


def test_scan_rounds(gpu):
    """alternating 1M 1X up to 255, 256, 257 and 513 runs (the scan works in rounds of 256 with a carry): counts and price exact"""
    cases = []
    for n in (255, 256, 257, 513):
        runs = [(1, "MX"[i & 1]) for i in range(n)]
        p, t = _spell(runs, 0x5C + n)
        c = Case("runs%d" % n, p, t, runs)
        assert c.expect["flags"] == 0 and c.expect["mismatches"] == n // 2 and c.expect["score"] == 5 * (n // 2) and c.expect["n_runs"] == n
        cases.append(c)
        # a wrong base in the last run, behind the carry
        tw = bytearray(t)
        tw[n - 1] = OTHER[tw[n - 1]] if (n - 1) % 2 == 0 else p[n - 1]
        cases.append(Case("runs%d_last" % n, p, bytes(tw), runs))
        assert cases[-1].expect["bad_run"] == n - 1
    # longer runs across several rounds, gaps among them
    runs = [((i * 7) % 23 + 1, "MXMIMD"[i % 6]) for i in range(700)]
    p, t = _spell(runs, 0x5D)
    cases.append(Case("mixed700", p, t, runs))
    assert cases[-1].expect["flags"] == 0
    _hold(gpu, cases)


def test_structural_flags(gpu):
    runs = [(10, "M"), (2, "X"), (9, "M"), (3, "I"), (12, "M")]
    p, t = _spell(runs, 0x51)
    cases = [
        Case("zero_length", p, t, runs[:1] + [(0, "D")] + runs[1:]),
        Case("adjacent_m", p, t, [(4, "M"), (6, "M")] + runs[1:]),
        Case("ops_len_minus", p, t, runs, ops_len=35),
        Case("ops_len_plus", p, t, runs, ops_len=37),
        Case("n_runs_minus", p, t, runs, n_runs=4),
        # one base short or over, either side; a wrong base sits in what an over-long problem must not compare
        Case("p_short", p + b"A", t, runs),
        Case("t_short", p, t + b"A", runs),
        Case("p_over", _wrong(p, 3)[:-1], t, runs),
        Case("t_over", p, _wrong(t, 3)[:-1], runs),
    ]
    want = {"zero_length": BAD_RUN, "adjacent_m": BAD_RUN, "ops_len_minus": COUNTS, "ops_len_plus": COUNTS, "n_runs_minus": COUNTS | SPANS,
            "p_short": SPANS, "t_short": SPANS, "p_over": SPANS, "t_over": SPANS}
    for c in cases:
        assert c.expect["flags"] == want[c.name], c.name
    assert cases[0].expect["bad_run"] == 1 and cases[1].expect["bad_run"] == 1
    _hold(gpu, cases)
    # a run range that leaves the run buffer is an argument error, not a read
    ss = gpu.upload([(p, t, UNI, 0, 0, 0, 0)])
    try:
        with pytest.raises(capi.WfmError):
            gpu.check_runs(ss, [(0, -1, 2, 36, 5)], np.array([(n << 2) | OPS.index(op) for n, op in runs], dtype=np.uint32))
    finally:
        ss.free()


def test_empty_sides_and_skipped(gpu):
    t10, p12 = synth.random_dna(0xE1, 10), synth.random_dna(0xE2, 12)
    skipped = dict.fromkeys(FIELDS, 0)
    skipped.update(flags=NOT_CHECKED, bad_p=-1, bad_t=-1)
    runs = [(12, "M")]
    cases = [
        Case("plen0", b"", t10, [(10, "I")]),
        Case("tlen0", p12, b"", [(12, "D")]),
        Case("both0", b"", b"", []),
        Case("score_only", p12, _wrong(p12, 4), [], mode=UNI | SO, score=5, ops_len=0, expect=skipped),
        Case("failed", p12, _wrong(p12, 4), runs, status=-300, score=-1, ops_len=0, expect=skipped),
        Case("after", p12, _wrong(p12, 4), runs),
    ]
    for c in cases[:3]:
        assert c.expect["flags"] == 0, c.name
    assert cases[0].expect["score"] == 8 + 2 * 10 and cases[1].expect["score"] == 8 + 2 * 12 and cases[2].expect["score"] == 0
    assert cases[-1].expect["flags"] == M_DIFFERS
    _hold(gpu, cases)


def test_bytes(gpu):
    """byte equality, nothing normalised: N equals N, a differs from A"""
    p = bytearray(synth.random_dna(0xB1, 60))
    p[7] = p[31] = ord("N")
    lower = bytearray(p)
    lower[40] = ord(chr(p[40]).lower())
    cases = [Case("n_n", p, p, [(60, "M")]), Case("a_A", p, lower, [(60, "M")])]
    assert cases[0].expect["flags"] == 0
    assert (cases[1].expect["flags"], cases[1].expect["bad_p"]) == (M_DIFFERS, 40)
    _hold(gpu, cases)


@pytest.mark.parametrize("pen", E.PENS, ids=lambda p: "default" if p is None else "-".join(map(str, p)))
def test_price(gpu, pen):
    """the correct score is clean, score +- 1 gives SCORE, score -1 is not compared: modes 0, 1, 2; mode 1 under the two patch tuples, a
    general tuple, and the op string of one run that uses both allowances of its side"""
    lead_d = [(6, "D"), (20, "M"), (2, "X"), (10, "M"), (30, "I"), (15, "M"), (1, "X"), (9, "M"), (40, "D"), (5, "M"), (4, "I")]
    lead_i = [(7, "I"), (18, "M"), (3, "D"), (11, "M"), (5, "D")]
    inner = [(25, "M"), (1, "X"), (14, "M")]
    todo = []
    for k, runs in enumerate((lead_d, lead_i, inner)):
        p, t = _spell(runs, 0x90 + k)
        todo += [(p, t, runs, M0, (0, 0, 0, 0)), (p, t, runs, UNI, (0, 0, 0, 0))]
        todo += [(p, t, runs, EF, f) for f in ((len(p), 0, len(t), 0), (0, len(p), 0, len(t)), (3, 4, 5, 6), (6, 0, 7, 2))]
    t10, p12 = synth.random_dna(0x9E, 10), synth.random_dna(0x9F, 12)
    todo += [(b"", t10, [(10, "I")], EF, (0, 0, 4, 3)), (b"", t10, [(10, "I")], EF, (0, 0, 10, 10)), (p12, b"", [(12, "D")], EF, (5, 2, 0, 0))]
    cases = []
    for k, (p, t, runs, mode, free) in enumerate(todo):
        true = _price(runs, mode, E.clamp(free, len(p), len(t)), pen)
        for claim, flag in ((true, 0), (true + 1, SCORE), (true - 1 if true > 0 else true + 2, SCORE), (-1, 0)):
            c = Case("%d_mode%d_%s_claim%d" % (k, mode, free, claim), p, t, runs, mode=mode, free=free, score=claim, pen=pen)
            assert c.expect["flags"] == flag and c.expect["score"] == true, c.name
            cases.append(c)
    x, o1, e1, o2, e2 = pen or E.DEFAULT_PEN
    # the single run under (0, 0, 4, 3): 10 - 4 - 3 bases are paid for
    single = [c for c in cases if c.runs == [(10, "I")] and c.free == (0, 0, 4, 3)]
    assert single and all(c.expect["score"] == min(o1 + 3 * e1, o2 + 3 * e2) for c in single)
    _hold(gpu, cases, pen)


def test_positive_pass_over_the_aligners(gpu):
    """the aligners' own output: ~60 ends-free problems of the family and ~40 end-to-end pairs (modes 0 and 2, up to ~3 kb); nothing is
    flagged and the price found equals the score reported"""
    fam = E.build_cases()
    items = [(c.p, c.t, EF) + tuple(c.free) for c in fam[::max(1, len(fam) // 60)]]
    for i in range(40):
        n = (40, 150, 700, 1500, 3000)[i % 5]
        p = synth.random_dna(0xAA00 + i, n)
        t = synth.mutate(p, (0.01, 0.05, 0.12)[i % 3], 0xAB00 + i)
        items.append((p, t, (M0, UNI)[i & 1], 0, 0, 0, 0))
    ss = gpu.upload(items)
    try:
        failed, runs = gpu.align_resident_rle(ss)
        assert failed == 0 and all(ss.results[i].status == 0 for i in range(ss.n))
        flagged, got = gpu.check_runs(ss, ss.results, runs)
        for i, g in enumerate(got):
            assert g.flags == 0, (i, g.flags, g.bad_p, g.bad_t, g.bad_run)
            assert g.score == ss.results[i].score, (i, g.score, ss.results[i].score)
            assert g.n_runs == ss.results[i].n_runs
            assert g.matches + g.mismatches + g.ins_bases + g.del_bases == ss.results[i].ops_len
        assert flagged == 0
    finally:
        ss.free()


def _revcomp(s):
    return bytes(s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")))


def test_upload_paths(gpu):
    """the same problems through wfm_upload_sequences and through wfm_upload_sequence_refs with text_revcomp = 1: identical results"""
    G = synth.random_dna(0xD0, 40000)
    H = _revcomp(G[100:39100])  # stored as it is; its windows come back reverse-complemented
    store = gpu.seqstore()
    try:
        gid, hid = store.add(G), store.add(H)
        wins = [(100, 39000, 0), (100, 37, 0), (5000, S + 9, 3), (133, 2 * S + 1, S + 2)]   # (start in G, length, a wrong base or 0)
        items, refs, words, results = [], [], [], []
        for start, n, wrong in wins:
            # G[start, start + n) is the reverse complement of H's window that ends at 39100 - start
            h0 = (39100 - start) - n
            text = _revcomp(H[h0:h0 + n])
            assert text == G[start:start + n]
            pat = bytearray(G[start:start + n])
            mode = UNI if n > 1000 else M0
            if wrong:
                # (the pattern side carries the wrong base: a host pointer in both uploads)
                pat[wrong] = OTHER[pat[wrong]]
            items.append((bytes(pat), text, mode, 0, 0, 0, 0))
            refs.append(dict(pattern=bytes(pat), text_seq=hid, text_off=h0, tlen=n, text_revcomp=1, mode=mode))
            results.append((0, -1, len(words), n, 1))
            words.append((n << 2) | 0)
        a, b = gpu.upload(items), gpu.upload_refs(store, refs)
        try:
            fa, ca = gpu.check_runs(a, results, np.array(words, dtype=np.uint32))
            fb, cb = gpu.check_runs(b, results, np.array(words, dtype=np.uint32))
        finally:
            a.free()
            b.free()
        assert fa == fb == sum(1 for w in wins if w[2])
        for (start, n, wrong), x, y in zip(wins, ca, cb):
            assert bytes(x) == bytes(y)
            assert (x.flags, x.bad_p, x.bad_t) == ((M_DIFFERS, wrong, wrong) if wrong else (0, -1, -1))
        assert gid == 0
    finally:
        store.free()
