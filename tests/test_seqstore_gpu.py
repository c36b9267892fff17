"""GPU tests of the device sequence store and of problems by reference: the seqset wfm_upload_sequence_refs lays out is the
one wfm_upload_sequences lays out for the same bases, byte for byte; aligning by reference gives what aligning the Python-made
strings gives (and the oracle); a bad reference is refused and the handle lives on; the align driver writes the same bytes
with resident_sequences as without."""
import os
import random
import subprocess

import pytest

from wfmash_amd import capi, synth
from oracle import wflign_host as W

pytestmark = pytest.mark.gpu

CH = capi.SEQ_GATHER_CHUNK
SEQ_PAD = 64  # wfa_host.hip
BI, EF, UNI = capi.WFM_MODE_END2END_BIWFA, capi.WFM_MODE_ENDSFREE, capi.WFM_MODE_END2END_UNI
CUSTOM_PEN = (4, 6, 2, 12, 1)


def _noisy(seed, n):
    """n bases with lower case, IUPAC letters and runs of N: what a FASTA holds before makeUpperCaseAndValidDNA."""
    rng = random.Random(seed)
    b = bytearray(synth.random_dna(seed, n))
    for _ in range(max(1, n // 400)):
        a = rng.randrange(0, n)
        e = min(n, a + rng.randrange(1, 40))
        kind = rng.randrange(3)
        if kind == 0:
            b[a:e] = bytes(b[a:e]).lower()
        elif kind == 1:
            b[a:e] = bytes(rng.choice(b"RYKMSWBDHVnx-") for _ in range(e - a))
        else:
            b[a:e] = b"N" * (e - a)
    return bytes(b)


# ---------------------------------------------------------------------------
# 1. byte parity of the layout
# ---------------------------------------------------------------------------
def _parity_problems(norm):
    """References and their Python-made twins.  Lengths, offsets and what lies before a problem are drawn so that every source
    and destination offset modulo 16 occurs; the caller asserts that they did."""
    rng = random.Random(11)
    lens = [0, 1, 15, 16, 17, 63, 64, 65, CH - 1, CH, CH + 1]
    refs, items = [], []

    def side(length_pool):
        sid = rng.randrange(len(norm))
        n = len(norm[sid])
        ln = rng.choice([x for x in length_pool if x <= n])
        where = rng.randrange(3)
        off = 0 if where == 0 else (n - ln if where == 1 else rng.randrange(0, n - ln + 1))
        rc = rng.randrange(2)
        s = norm[sid][off:off + ln]
        return sid, off, ln, rc, (W.revcomp(s) if rc else s)

    def put(ps, po, pl, prc, ts, to, tl, trc, mode, free):
        p, t = norm[ps][po:po + pl], norm[ts][to:to + tl]
        refs.append(dict(pattern_seq=ps, pattern_off=po, plen=pl, pattern_revcomp=prc, text_seq=ts, text_off=to, tlen=tl, text_revcomp=trc,
                         mode=mode, pattern_begin_free=free[0], pattern_end_free=free[1], text_begin_free=free[2], text_end_free=free[3]))
        items.append((W.revcomp(p) if prc else p, W.revcomp(t) if trc else t, mode) + free)

    # every length on both sides and both strands as a BiWFA problem (forward and reversed copies), cut from the long sequence
    n3 = len(norm[3])
    for ln in lens:
        for rc in (0, 1):
            put(3, rng.randrange(0, n3 - ln + 1), ln, rc, 3, rng.randrange(0, n3 - ln + 1), ln, 1 - rc, BI, (0, 0, 0, 0))
    for i in range(200):
        pool = lens[:8] + [rng.randrange(0, 300)]
        ps, po, pl, prc, p = side(pool)
        ts, to, tl, trc, t = side(pool)
        if i % 7 == 0:  # the same sequence on both sides
            ts = ps
            tl = min(tl, len(norm[ts]))
            to = rng.randrange(0, len(norm[ts]) - tl + 1)
        mode = (BI, EF, UNI)[i % 3]
        free = (pl, 0, tl, 0) if i % 2 else (0, pl, 0, tl)
        if mode != EF:
            free = (0, 0, 0, 0)
        put(ps, po, pl, prc, ts, to, tl, trc, mode, free)
    return refs, items


def test_layout_is_byte_identical_to_the_host_upload(gpu):
    raw = [_noisy(101, 1), _noisy(102, 37), _noisy(103, 5000), _noisy(104, 2 * CH + 33)]
    norm = [W.upper_valid_dna(s) for s in raw]
    assert any(c in raw[3] for c in b"acgtn") and any(c in raw[3] for c in b"RYKM") and b"NNNN" in raw[3]
    store = gpu.seqstore()
    try:
        assert [store.add(s) for s in raw] == [0, 1, 2, 3]
        n_seqs, nbytes = store.info()
        assert n_seqs == 4 and nbytes >= sum(len(s) + 32 for s in raw)  # 16 bytes of slack and more on either side
        refs, items = _parity_problems(norm)
        # coverage is a condition: offsets modulo 16 on both ends of the copy, the lengths, the edges, the flags, the modes
        src_mod, dst_mod, at = set(), set(), SEQ_PAD
        for r in refs:
            for off, ln in ((r["pattern_off"], r["plen"]), (r["text_off"], r["tlen"])):
                if ln:
                    src_mod.add(off % 16)
                    dst_mod.add(at % 16)
                at += ln + SEQ_PAD
        assert src_mod == set(range(16)) and dst_mod == set(range(16))
        for ln in (0, 1, 15, 16, 17, 63, 64, 65, CH - 1, CH, CH + 1):
            assert any(r["plen"] == ln for r in refs) and any(r["tlen"] == ln for r in refs), ln
        assert any(r["pattern_off"] == 0 and r["plen"] > 16 for r in refs)
        assert any(r["text_off"] + r["tlen"] == len(norm[r["text_seq"]]) and r["tlen"] > 16 for r in refs)
        assert {(r["pattern_revcomp"], r["text_revcomp"]) for r in refs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert any(r["pattern_seq"] == r["text_seq"] for r in refs) and {r["mode"] for r in refs} == {BI, EF, UNI}
        for rc in (0, 1):  # a window of several tasks, forward and reversed copy, from either strand
            assert any(r["mode"] == BI and r["plen"] > CH and r["pattern_revcomp"] == rc for r in refs)
        a = gpu.upload(items)
        b = gpu.upload_refs(store, refs)
        try:
            want, got = a.download(), b.download()
        finally:
            a.free()
            b.free()
        assert len(want) == len(got) and len(want) > 4 * CH
        if want != got:
            first = next(i for i in range(len(want)) if want[i] != got[i])
            raise AssertionError(f"the seqsets differ from byte {first} of {len(want)}: {want[first:first + 24]!r} != {got[first:first + 24]!r}")
    finally:
        store.free()


# ---------------------------------------------------------------------------
# 2. - 4. results
# ---------------------------------------------------------------------------
class _Case:
    pass


@pytest.fixture(scope="module")
def case(gpu):
    """About 40 pairs of 200 - 6000 bases and two longer than a gather chunk, 2 - 5 % apart, half of them with the query on the
    reverse strand, a few with an N; the targets end to end in one stored sequence, the queries -- as the file holds them, i.e.
    reverse-complemented where the record is '-' -- in another.  Head and tail patches of some pairs as ends-free sub-windows."""
    rng = random.Random(23)
    c = _Case()
    lens = [rng.randrange(200, 6001) for _ in range(40)] + [CH + 700, CH + 3500]
    tchr, qchr = bytearray(), bytearray()
    c.refs, c.items, c.mixed_a, c.mixed_b = [], [], [], []
    pairs = []
    for i, L in enumerate(lens):
        t = bytearray(synth.random_dna(9000 + i, L))
        q = bytearray(synth.mutate(bytes(t), rng.choice([0.02, 0.03, 0.05]), 9500 + i))
        if i % 9 == 4:  # an N (or what becomes one) on either side
            t[L // 3] = ord("N")
            q[len(q) // 2] = ord("r")
        rev = i % 2 == 1
        to, qo = len(tchr) + rng.randrange(0, 23), len(qchr) + rng.randrange(0, 23)
        tchr += synth.random_dna(9900 + i, to - len(tchr)) + bytes(t)
        qchr += synth.random_dna(9950 + i, qo - len(qchr)) + (W.revcomp(W.upper_valid_dna(bytes(q))) if rev else bytes(q))
        pairs.append((to, L, qo, len(q), rev))
    c.raw = [bytes(tchr), bytes(qchr)]
    norm = [W.upper_valid_dna(s) for s in c.raw]

    def add(to, pl, qo, ql, rev, a_t, b_t, a_q, b_q, mode, free, hint=0):
        """bases [a_t, b_t) of the target window against [a_q, b_q) of the strand-adjusted query window"""
        p = norm[0][to:to + pl][a_t:b_t]
        qwin = norm[1][qo:qo + ql]
        t = (W.revcomp(qwin) if rev else qwin)[a_q:b_q]
        q_off = qo + ql - b_q if rev else qo + a_q
        fr = dict(pattern_begin_free=free[0], pattern_end_free=free[1], text_begin_free=free[2], text_end_free=free[3])
        c.refs.append(dict(pattern_seq=0, pattern_off=to + a_t, plen=b_t - a_t, text_seq=1, text_off=q_off, tlen=b_q - a_q,
                           text_revcomp=int(rev), mode=mode, **fr))
        c.mixed_a.append(dict(pattern_seq=0, pattern_off=to + a_t, plen=b_t - a_t, text=t, mode=mode, **fr))
        c.mixed_b.append(dict(pattern=p, text_seq=1, text_off=q_off, tlen=b_q - a_q, text_revcomp=int(rev), mode=mode, **fr))
        c.items.append((p, t, mode) + tuple(free))

    for i, (to, pl, qo, ql, rev) in enumerate(pairs):
        add(to, pl, qo, ql, rev, 0, pl, 0, ql, BI, (0, 0, 0, 0))
        if i % 4 == 0:  # head_problem: the first bases, begin-free; tail_problem: the last, end-free (wflign_hip.cpp)
            a, b = min(pl, rng.randrange(130, 700)), min(ql, rng.randrange(130, 700))
            add(to, pl, qo, ql, rev, 0, a, 0, b, EF, (a, 0, b, 0))
            add(to, pl, qo, ql, rev, pl - a, pl, ql - b, ql, EF, (0, a, 0, b))
    c.store = gpu.seqstore()
    assert [c.store.add(s) for s in c.raw] == [0, 1]
    c.want = {}
    for pen in (None, CUSTOM_PEN):
        res = gpu.align(c.items, pen)
        c.want[pen] = (res, gpu.problem_flags(len(c.items)).copy())
    yield c
    c.store.free()


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g.status, g.score) == (w.status, w.score), i
        assert g.ops == w.ops, i


@pytest.mark.parametrize("pen", [None, CUSTOM_PEN])
def test_align_refs_equals_align_on_strings(gpu, oracle, case, pen):
    want, want_flags = case.want[pen]
    assert sum(r.status == 0 for r in want) == len(want) >= 60
    got = gpu.align_refs(case.store, case.refs, pen)
    flags = gpu.problem_flags(len(case.refs))
    _same(got, want)
    assert (flags == want_flags).all()
    assert any(f & capi.WFM_PF_BYTE_KERNEL for f in flags)  # the records with an N
    # a dozen against the oracle as well, the two long records among them
    n = len(case.items)
    for i in sorted(set(range(0, n, max(1, n // 10))) | {j for j in range(n) if len(case.items[j][0]) > CH}):
        p, t, mode = case.items[i][:3]
        if mode == BI:
            rc, ops, sc, _ = oracle.align_biwfa(p, t, pen)
        else:
            pbf, pef, tbf, tef = case.items[i][3:7]
            rc, ops, sc, _ = oracle.align_endsfree(p, pbf, pef, t, tbf, tef, pen)
        assert rc == 0 and got[i].score == sc and got[i].ops == ops, i


@pytest.mark.parametrize("which", ["pattern_from_store", "text_from_store"])
def test_mixed_sides(gpu, case, which):
    """one side a window of the store, the other a host pointer: only that one crosses PCIe, the results are the same"""
    refs = case.mixed_a if which == "pattern_from_store" else case.mixed_b
    _same(gpu.align_refs(case.store, refs), case.want[None][0])


def test_bad_references_are_refused_and_the_handle_lives_on(gpu, case):
    n_t, n_q = len(case.raw[0]), len(case.raw[1])
    good = dict(pattern_seq=0, pattern_off=0, plen=500, text_seq=1, text_off=0, tlen=500)
    for change in (dict(pattern_off=n_t - 499),          # one base past the end
                   dict(text_off=n_q - 499),
                   dict(pattern_off=-1),                   # a negative offset
                   dict(text_off=-5),
                   dict(pattern_seq=2),                    # an unknown id
                   dict(text_seq=-2),
                   dict(text_seq=-1, text=None)):          # a host side of non-zero length without its bytes
        with pytest.raises(capi.WfmError):
            gpu.align_refs(case.store, [good, dict(good, **change)])
        assert gpu.last_error()
    with pytest.raises(capi.WfmError):  # windows of a store without a store
        gpu.align_refs(None, [good])
    # the last base is still inside
    r = gpu.align_refs(case.store, [dict(good, pattern_off=n_t - 500)])
    assert r[0].status == 0
    _same(gpu.align_refs(case.store, case.refs[:12]), case.want[None][0][:12])


# ---------------------------------------------------------------------------
# 5. the align driver
# ---------------------------------------------------------------------------
def _write_fasta(path, seqs, width=60):
    with open(path, "wt") as f:
        for name, s in seqs.items():
            f.write(f">{name} some description\n")
            s = s.decode()
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + "\n")


@pytest.fixture(scope="module")
def driver_case(tmp_path_factory):
    """A small pangenome in the manner of tests/test_align_paf_gpu.py (lower case and IUPAC in one haplotype, one haplotype
    reverse-complemented, chains of several pieces) and, in a mapping file of their own that is run without padding, records
    whose target carries 500 extra bases shortly before its end.  With 30 bases behind them the main alignment ends 500D,30=,
    but the tail scan does not stop before it has 128 bases (MIN_PATCH_LENGTH, wflign.cpp:169), takes the gap along, and the
    ends-free tail patch leaves the record ending 30I,530D: no bases are read for it.  With 200 bases behind them the scan
    stops on the final run and the record ends 500D,200=, which is where the swizzle reads bases.  Two records of each kind, one
    per strand; what each ends in is confirmed with oracle/wflign_host.py here, on the CPU, before any test relies on it."""
    tmp = tmp_path_factory.mktemp("resident")
    seed, L = 41, 20000
    rng = random.Random(seed)
    base = synth.random_dna(seed, L)
    seqs = {}
    for h in range(4):
        s = synth.mutate(base, rng.choice([0.01, 0.03, 0.06]), seed * 100 + h)
        if h == 1:
            b = bytearray(s)
            b[5000:5200] = bytes(b[5000:5200]).lower()
            b[9000:9005] = b"RYKMN"
            s = bytes(b)
        seqs[f"hap{h}#1#chr1"] = s
    seqs["hap9#1#chr1"] = W.revcomp(synth.mutate(base, 0.04, seed * 100 + 9))
    names = list(seqs)
    lines = []
    chain = 0
    for _ in range(20):
        qn, tn = rng.sample(names, 2)
        qlen_total, tlen_total = len(seqs[qn]), len(seqs[tn])
        seg = rng.choice([1500, 4000, 9000])
        qs = rng.randrange(0, min(qlen_total, tlen_total) - seg - 600)
        qe = qs + seg
        rev = (qn == "hap9#1#chr1") != (tn == "hap9#1#chr1")
        ts, te = (tlen_total - qe, tlen_total - qs) if rev else (qs, qe)
        ts = max(0, ts + rng.randrange(-60, 60))
        te = min(tlen_total, te + rng.randrange(-60, 60))
        chain += 1
        n_pieces = rng.choice([1, 1, 2, 3])
        cuts_q = [qs + (qe - qs) * k // n_pieces for k in range(n_pieces + 1)]
        cuts_t = [ts + (te - ts) * k // n_pieces for k in range(n_pieces + 1)]
        for k in range(n_pieces):
            tq0, tq1 = (cuts_t[n_pieces - k - 1], cuts_t[n_pieces - k]) if rev else (cuts_t[k], cuts_t[k + 1])
            lines.append("\t".join(map(str, [qn, qlen_total, cuts_q[k], cuts_q[k + 1], "-" if rev else "+", tn, tlen_total,
                                             tq0, tq1, 100, seg, 30, "id:f:0.95", "kc:f:0.9", f"ch:Z:{chain}.{k + 1}.{n_pieces}"])))
    lines.append("garbage line with too few columns")
    # the records of the second file: hap0 (and its reverse complement) against hap0 with 500 bases put in shortly before the window's end
    h0 = seqs["hap0#1#chr1"]
    E = 15000
    seqs["rc0#1#chr1"] = W.revcomp(h0)
    zero, n_lazy = [], 0
    for behind in (30, 200):
        tn = f"ins{behind}#1#chr1"
        seqs[tn] = h0[:E - behind] + synth.random_dna(777, 500) + h0[E - behind:]
        for qn, S, rev in (("hap0#1#chr1", E - 6000, False), ("rc0#1#chr1", E - 9000, True)):
            q0, q1 = (len(h0) - E, len(h0) - S) if rev else (S, E)
            zero.append("\t".join(map(str, [qn, len(h0), q0, q1, "-" if rev else "+", tn, len(seqs[tn]), S, E + 500,
                                            100, E - S, 30, "id:f:0.99", "kc:f:0.9", f"ch:Z:{90 + len(zero)}.1.1"])))
            tav = W.upper_valid_dna(seqs[tn][S:])
            cg = W.parse(W.do_biwfa_alignment(W.upper_valid_dna(h0[S:E]), tav[:E + 500 - S], tav))
            ends = [op for _, op in cg[-2:]]
            if behind == 200:
                assert ends == ["D", "="] and cg[-2][0] == 500, cg[-3:]
                n_lazy += 1
            else:
                assert ends == ["I", "D"] and [op for _, op in cg[:2]] != ["=", "D"], cg
    c = _Case()
    c.fa = str(tmp / "pan.fa")
    _write_fasta(c.fa, seqs)
    c.paf, c.paf_zero = str(tmp / "map.paf"), str(tmp / "zero.paf")
    for path, ls in ((c.paf, lines), (c.paf_zero, zero)):
        with open(path, "w") as f:
            f.write("\n".join(ls) + "\n")
    c.tmp, c.seqs, c.n_main, c.n_zero, c.n_lazy_zero = tmp, seqs, len(lines) - 1, len(zero), n_lazy
    return c


ZERO_PAD = {"target_padding": 0, "query_padding": 0}


def _run(gpu, c, paf, name, **params):
    out = str(c.tmp / name)
    summ = capi.align_paf(gpu, c.fa, paf, out, params=params)
    return open(out, "rb").read(), summ


def test_driver_writes_the_same_paf_and_fetches_lazily(gpu, driver_case):
    c = driver_case
    want, s0 = _run(gpu, c, c.paf, "main.paf")
    got, s1 = _run(gpu, c, c.paf, "main_res.paf", resident_sequences=1)
    assert want.count(b"\n") >= 20 and s0.records == c.n_main and s0.skipped == 1
    assert (s0.records_resident, s0.lazy_fetches) == (0, 0)  # the switch is off
    assert got == want
    assert s1.records == c.n_main and s1.records_resident == s1.records
    wantz, z0 = _run(gpu, c, c.paf_zero, "zero_out.paf", **ZERO_PAD)
    gotz, z1 = _run(gpu, c, c.paf_zero, "zero_out_res.paf", resident_sequences=1, **ZERO_PAD)
    assert wantz.count(b"\n") == c.n_zero == 4 and gotz == wantz
    assert z1.records_resident == z1.records == c.n_zero
    assert z1.lazy_fetches == c.n_lazy_zero == 2  # the two that end D,=: the swizzle needs their bases
    assert 0 < s1.lazy_fetches + z1.lazy_fetches < s1.records + z1.records


def test_driver_sam_with_md(gpu, driver_case):
    c = driver_case
    want, _ = _run(gpu, c, c.paf, "main.sam", sam_format=1, emit_md_tag=1)
    got, s = _run(gpu, c, c.paf, "main_res.sam", sam_format=1, emit_md_tag=1, resident_sequences=1)
    assert want.count(b"\n") >= 20 and b"MD:Z:" in want
    assert got == want
    assert s.records_resident == s.records == c.n_main


def test_driver_budget_leaves_sequences_on_the_host(gpu, driver_case, monkeypatch):
    """WFM_SEQSTORE_GB is read when the store is made: a budget of one and a half sequences holds the first one that is asked
    for, the sides of every other sequence stay host pointers, the bytes are the same."""
    c = driver_case
    want, _ = _run(gpu, c, c.paf, "main_b.paf")
    monkeypatch.setenv("WFM_SEQSTORE_GB", "%.12f" % (30000 / 2.0 ** 30))
    got, s = _run(gpu, c, c.paf, "main_b_res.paf", resident_sequences=1)
    assert got == want
    assert s.records == c.n_main and s.records_resident < s.records


def test_driver_two_handles_of_one_device_share_the_store(gpu, driver_case):
    c = driver_case
    want, _ = _run(gpu, c, c.paf, "main_m.paf")
    other = capi.Handle(0)
    try:
        out = str(c.tmp / "main_m_res.paf")
        s = capi.align_paf_multi([gpu, other], c.fa, c.paf, out, params={"resident_sequences": 1})
        assert open(out, "rb").read() == want
        assert s.records_resident == s.records == c.n_main
    finally:
        other.close()


def test_cli_switch(driver_case):
    c = driver_case
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wfmash_amd", "wfmash-hip")
    outs = []
    for extra in ([], ["--resident-seqs"]):
        out = str(c.tmp / ("cli%d.paf" % len(extra)))
        r = subprocess.run([cli, "-i", c.paf, "-t", "4", "--out", out, c.fa] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(open(out, "rb").read())
    assert outs[0].count(b"\n") >= 20 and outs[0] == outs[1]
