"""GPU tests of --chain: wfm_chain_runs word for word against the brute-force model (tests/chain_model.py) on hand cases, the 256-run
rounds, blocks and gaps that cross them, refused problems and calls, chunked output and a seeded fuzz; then the align driver on the
synthetic pangenome of tests/test_left_align_gpu.py and the command line."""
import os
import random
import re
import subprocess
import types

import pytest

from tests import chain_model as M
from tests import lift_model as LM
from tests import test_left_align_gpu as LT  # its synthetic pangenome (nothing of it is collected from here)
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
SPANS = capi.WFM_CHAIN_SPANS
P = LM.parse


# ---- 1. the C ABI against the model ----
def _layout(problems, junk=0, reverse=False):
    """the run buffer and [(runs_off, n_runs, flags)]: `junk` words of rubbish before, between and behind the problems' runs; reverse: the
    problems' runs lie in the buffer in the opposite order, so runs_off descends"""
    rubbish = [0xFFFFFFFF, 0, 7, (5 << 2) | 3]
    buf, where = [], [None] * len(problems)
    order = range(len(problems) - 1, -1, -1) if reverse else range(len(problems))
    for k in order:
        buf += [rubbish[(k + j) % 4] for j in range(junk)]
        where[k] = (len(buf), len(problems[k][0]), problems[k][1])
        buf += LM.words(problems[k][0])
    buf += rubbish[:junk]
    return buf, where


def _chain(gpu, problems, junk=0, reverse=False):
    """(blocks, per) of one call as lists of tuples like the model's, and the blocks' bytes"""
    buf, where = _layout(problems, junk, reverse)
    blocks, per = gpu.chain_runs(where, buf)
    return blocks.tolist(), per.tolist(), blocks.tobytes() + per.tobytes()


def _assert_model(gpu, problems, **kw):
    blocks, per, _ = _chain(gpu, problems, **kw)
    want_blocks, want_per = M.chain_problems(problems)
    assert per == want_per
    assert blocks == want_blocks
    return blocks, per


HAND = ["7=", "7X", "7I", "7D", "2I3D1I", "2I5=", "2D5=", "5=2I", "5=2D", "2I5=2D", "2D5=2I", "1I2D5=3D1I", "3D1I2D4=1X1I", "1=1X1=1X", "3=2X4=",
        "4=3D4=", "4=2I3D4=", "4=3D2I4=", "4=2I4=1X3D2=1I1D1I7=", "1I1=1D1X1I1=1D", "2D1=1I1=1D1=2I"]


@pytest.mark.parametrize("cigar", HAND)
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_hand_cases_word_for_word(gpu, cigar, flags):
    _, per = _assert_model(gpu, [(P(cigar), flags)])
    assert per[0][0] == 0


def test_hand_cases_spelled_out(gpu):
    """a few of the above against numbers written by hand, not the model's"""
    got = lambda c, f=0: _chain(gpu, [(P(c), f)])[:2]
    assert got("4=3D4=") == ([(4, 3, 0, 4), (4, 0, 0, 4)], [(0, 3, 0, 2, 0, 0, 0, 0, 8, 0)])
    assert got("4=2I3D4=")[0] == [(4, 3, 2, 4), (4, 0, 0, 4)] and got("4=3D2I4=")[0] == [(4, 3, 2, 4), (4, 0, 0, 4)]
    assert got("2I5=2D") == ([(5, 0, 0, 5)], [(0, 3, 0, 1, 0, 2, 2, 0, 5, 0)])
    assert got("3=2X4=") == ([(9, 0, 0, 7)], [(0, 3, 0, 1, 0, 0, 0, 0, 7, 2)])
    assert got("2I3D1I") == ([], [(0, 3, 0, 0, 3, 3, 0, 0, 0, 0)])
    # 3= (1D, 2I) 1X (4D, 0I) 2=, lead 1I, trail 5D
    c = "1I3=1D2I1X4D2=5D"
    assert got(c, 0) == ([(3, 1, 2, 3), (1, 4, 0, 0), (2, 0, 0, 2)], [(0, 8, 0, 3, 0, 1, 5, 0, 5, 1)])
    assert got(c, 1) == ([(3, 2, 1, 3), (1, 0, 4, 0), (2, 0, 0, 2)], [(0, 8, 0, 3, 1, 0, 0, 5, 5, 1)])
    assert got(c, 2) == ([(2, 4, 0, 2), (1, 1, 2, 0), (3, 0, 0, 3)], [(0, 8, 0, 3, 5, 0, 0, 1, 5, 1)])
    assert got(c, 3) == ([(2, 0, 4, 2), (1, 2, 1, 0), (3, 0, 0, 3)], [(0, 8, 0, 3, 0, 5, 1, 0, 5, 1)])


def _mixed(n_runs, seed, ends="="):
    """n_runs runs of all four ops, never two of a kind in a row; ends: aligned at both ends, or anything (None)"""
    rng = random.Random(seed)
    runs, last = [], None
    for k in range(n_runs):
        op = rng.choice([o for o in "=XID" if o != last]) if (0 < k < n_runs - 1 or ends is None) else ends
        if op == last:
            op = "X" if op == "=" else "="
        runs.append((rng.randrange(1, 4), op))
        last = op
    return runs


@pytest.mark.parametrize("n_runs", [1, 255, 256, 257, 1025])
def test_run_counts_on_the_round_carry(gpu, n_runs):
    _assert_model(gpu, [(_mixed(n_runs, n_runs + f, None if f & 1 else "="), f) for f in range(4)])


def test_blocks_and_gaps_across_the_rounds(gpu):
    one_block = P("1=1X") * 300                       # 600 runs, one block over three rounds
    one_gap = P("5=") + P("1I1D") * 600 + P("5=")     # a gap over three rounds (and a half)
    lane_255_then_0 = P("1D1I") * 127 + P("1D") + P("3=") + P("2X") + P("4I") + P("1D1I") * 127 + P("6=")
    assert lane_255_then_0[255][1] == "=" and lane_255_then_0[254][1] == "D" and lane_255_then_0[512][1] == "=" and lane_255_then_0[511][1] == "I"
    head_in_lane_0 = P("1D1I") * 128 + P("3=1D2=")
    assert head_in_lane_0[256][1] == "="
    problems = [(r, f) for r in (one_block, one_gap, lane_255_then_0, head_in_lane_0) for f in range(4)]
    blocks, per = _assert_model(gpu, problems)
    assert per[0][3] == 1 and blocks[0] == (600, 0, 0, 300)
    assert per[4][3] == 2 and blocks[per[4][2]] == (5, 600, 600, 5)


def test_single_run_blocks_under_reverse(gpu):
    """1024 blocks of one run each: under REVERSE every output slot lies on the other side of a round boundary from its head"""
    runs = P("1=1D") * 1024
    blocks, per = _assert_model(gpu, [(runs, 2), (runs, 0), (runs, 3)])
    assert per[0][3] == 1024 and per[0][4:8] == (1, 0, 0, 0) and blocks[0] == (1, 1, 0, 1) and blocks[1023] == (1, 0, 0, 1)
    assert blocks[2048] == (1, 0, 1, 1)


def test_ten_thousand_alternating_gaps(gpu):
    blocks, _ = _assert_model(gpu, [(P("5=") + P("1I1D") * 10000 + P("5="), 0)])
    assert blocks == [(5, 10000, 10000, 5), (5, 0, 0, 5)]


def _many(seed=0xBEEF, n_prob=60):
    rng = random.Random(seed)
    return [(_mixed(rng.randrange(1, 90), seed + k, None), rng.randrange(4)) for k in range(n_prob)]


def test_junk_between_the_runs_and_descending_offsets(gpu):
    problems = _many()
    a, _ = _assert_model(gpu, problems, junk=5)
    b, _ = _assert_model(gpu, problems, junk=3, reverse=True)
    assert a == b and len(a) > 300


def test_refused_problems_leave_their_neighbours_alone(gpu):
    good = [(P("10="), 0), (P("4=2D1I9="), 3), (P("2I10=1D3X"), 2)]
    wide = [(2, "=")] + [((1 << 30) - 1, "I")] * 4 + [(2, "I")]  # a text span of 2^32 exactly; the pattern span is two bases
    assert sum(n for n, _ in wide) == 1 << 32
    fits = wide[:-1] + [(1, "I")]
    bad = [(P("3=0D2="), 0), ([], 1), (wide, 0), ([(n, "D" if op == "I" else op) for n, op in wide], 2)]
    problems = [good[0], bad[0], bad[1], good[1], bad[2], bad[3], good[2], (fits, 0)]
    # (the model refuses before it expands; the last one is legal and too long to expand: its answer by hand)
    buf, where = _layout(problems)
    blocks, per = gpu.chain_runs(where, buf)
    blocks, per = blocks.tolist(), per.tolist()
    want_blocks, want_per = M.chain_problems(problems[:-1])
    assert per[:-1] == want_per and per[-1] == (0, 6, len(want_blocks), 1, 0, 0, 0, (1 << 32) - 3, 2, 0)
    assert blocks == want_blocks + [(2, 0, 0, 2)]
    assert [p[0] for p in per] == [0, SPANS, SPANS, 0, SPANS, SPANS, 0, 0] and all(p[3:] == (0,) * 7 for p in per if p[0])
    alone, _, _ = _chain(gpu, good)
    assert blocks[:-1] == alone


def test_a_run_range_past_the_buffer(gpu):
    words = LM.words(P("10="))
    for where in ([(0, 2, 0)], [(1, 1, 0)], [(0, 1, 0), (5, 1, 0)], [(2, 0, 0)]):
        with pytest.raises(capi.WfmError, match="leave the run buffer"):
            gpu.chain_runs(where, words)
    blocks, per = gpu.chain_runs([(0, 1, 0)], words)  # the handle is usable afterwards
    assert blocks.tolist() == [(10, 0, 0, 10)] and per.tolist() == [(0, 1, 0, 1, 0, 0, 0, 0, 10, 0)]


def test_an_unknown_flag_bit(gpu):
    words = LM.words(P("10="))
    for flags in (4, 7, 1 << 31):
        with pytest.raises(capi.WfmError, match=r"\(-3\).*neither WFM_CHAIN_SWAP nor WFM_CHAIN_REVERSE"):
            gpu.chain_runs([(0, 1, 0), (0, 1, flags)], words)
    assert gpu.chain_runs([(0, 1, 3)], words)[0].tolist() == [(10, 0, 0, 10)]


def test_no_problems_and_no_blocks(gpu):
    blocks, per = gpu.chain_runs([], [])
    assert len(blocks) == 0 and len(per) == 0
    blocks, per, _ = _chain(gpu, [(P("3I2D"), 0), (P("1D"), 3)])
    assert blocks == [] and per == [(0, 2, 0, 0, 2, 3, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0, 1, 0, 0)]
    # the C call itself: WFM_OK, NULL and 0
    import ctypes as C
    ptr, n = C.c_void_p(1), C.c_size_t(1)
    assert gpu._L.wfm_chain_runs(gpu._p, None, 0, None, 0, C.byref(ptr), C.byref(n), None) == 0 and not ptr.value and n.value == 0


def test_chunked_output_is_the_same_bytes(gpu, monkeypatch):
    problems = _many(seed=0xC0DE)
    blocks, per, raw = _chain(gpu, problems)
    assert len(blocks) > 300 and max(p[3] for p in per) > 8
    monkeypatch.setenv("WFM_CHAIN_OUT_MB", "0.00002")  # one block: every problem a chunk of its own, most of them larger than that
    assert _chain(gpu, problems)[2] == raw
    monkeypatch.setenv("WFM_CHAIN_OUT_MB", "0.001")
    assert _chain(gpu, problems)[2] == raw


def test_two_calls_give_the_same_bytes(gpu):
    problems = _many(seed=0xFACE)
    a, b = _chain(gpu, problems), _chain(gpu, problems)
    assert a[2] == b[2] and len(a[0])


def test_fuzz_equals_the_model(gpu):
    rng = random.Random(0x11F7)
    problems = [(_mixed(rng.choice([rng.randrange(1, 40), rng.randrange(1, 701)]), 77 + k, None), rng.randrange(4)) for k in range(300)]
    blocks, per = _assert_model(gpu, problems, junk=2)
    assert len(blocks) > 5000 and max(p[1] for p in per) > 600


def test_interleaved_with_lift_and_cs_on_one_handle(gpu):
    """chain_runs shares the handle's scratch and output blocks with the other record passes: small, large, small again on ONE handle,
    between lift and cs_strings, against fresh handles"""
    from wfmash_amd import synth

    def batch(seed, n, length):
        items = []
        for i in range(n):
            t = synth.random_dna(seed + i, length + 7 * i)
            items.append((t, synth.mutate(t, 0.06, (seed << 8) + i, p_sub=0.6, p_ins=0.2)))
        return items

    def passes(h, items):
        ss = h.upload(items)
        s = h.liftset([(0, 1 << 20), (100, 200)], 1 << 20)
        try:
            failed, runs = h.align_resident_rle(ss)
            assert failed == 0
            res = ss.results[:ss.n]
            lifts, lper = s.lift([(0, r.ops_off, r.n_runs) for r in res], runs)
            blocks, per = h.chain_runs([(r.ops_off, r.n_runs, k % 4) for k, r in enumerate(res)], runs)
            short, _ = h.cs_strings(ss, ss.results, runs, capi.WFM_CS_SHORT)
            blocks2, per2 = h.chain_runs([(r.ops_off, r.n_runs, 0) for r in res], runs)
            want = M.chain_problems([([(w >> 2, "=XID"[w & 3]) for w in runs[r.ops_off:r.ops_off + r.n_runs].tolist()], 0) for r in res])
            assert (blocks2.tolist(), per2.tolist()) == want
            return lifts.tobytes(), lper.tobytes(), blocks.tobytes(), per.tobytes(), short, blocks2.tobytes()
        finally:
            s.close()
            ss.free()

    small, large = batch(0x6a00, 3, 300), batch(0x6b00, 40, 2000)
    want = {}
    for name, items in (("small", small), ("large", large)):
        h = capi.Handle(0)
        try:
            want[name] = passes(h, items)
        finally:
            h.close()
    assert len(want["large"][2]) > len(want["small"][2]) > 0
    for name, items in (("small", small), ("large", large), ("small", small)):
        got = passes(gpu, items)
        for k, (g, w) in enumerate(zip(got, want[name])):
            assert g == w, (name, k)


# ---- 2. the align driver ----
def _align(handles, case, out, chain, swap=False, left=False, **params):
    capi.set_chain(chain, swap)
    capi.set_left_align(left)
    try:
        if len(handles) == 1:
            capi.align_paf(handles[0], case.fa, case.paf, out, params=params or None)
        else:
            capi.align_paf_multi(handles, case.fa, case.paf, out, params=params or None)
        return open(out, "rb").read(), (open(chain, "rb").read() if chain else None), capi.chain_counts()
    finally:
        capi.set_chain(None)
        capi.set_left_align(False)


def _records_of(paf_lines):
    """the PAF's own records as chain_model.chain_text takes them"""
    out = []
    for line in paf_lines:
        f = line.rstrip("\n").split("\t")
        out.append(dict(qname=f[0], qsize=int(f[1]), qs=int(f[2]), qe=int(f[3]), strand=f[4], tname=f[5], tsize=int(f[6]), ts=int(f[7]), te=int(f[8]),
                        runs=P([v for v in f[12:] if v.startswith("cg:Z:")][0][5:])))
    return out


def _counts_of(text):
    chains = M.parse_chains(text)
    return (len(chains), sum(len(b) for _, b in chains), 0, 0)


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows, the aligned PAF of a run without the switch and the chain file of one with it: made once, never
    changed"""
    d = str(tmp_path_factory.mktemp("chain"))
    fa, paf, seqs = LT._make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, seqs=seqs)
    c.text, none, counts = _align([gpu], c, os.path.join(d, "plain.paf"), None)
    assert none is None and counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20
    c.with_text, c.chain, c.counts = _align([gpu], c, os.path.join(d, "with.paf"), os.path.join(d, "with.chain"))
    return c


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _side(seqs, name, strand, start, end):
    s = seqs[name]
    s = s.encode() if isinstance(s, str) else s
    return (s.translate(_COMP)[::-1] if strand == "-" else s)[start:end].upper()


def test_driver_plain(gpu, case):
    assert case.with_text == case.text
    want = M.chain_text(_records_of(case.lines))
    assert case.chain == want and case.counts == _counts_of(want)
    chains = M.parse_chains(case.chain)
    assert [h["id"] for h, _ in chains] == list(range(1, len(case.lines) + 1))  # every record has a chain; the ids are 1 .. n in file order
    assert {h["qstrand"] for h, _ in chains} == {"+", "-"} and max(len(b) for _, b in chains) > 3
    for (head, blocks), line in zip(chains, case.lines):
        assert sum(b[0] + b[1] for b in blocks) == head["tend"] - head["tstart"] and sum(b[0] + b[2] for b in blocks) == head["qend"] - head["qstart"]
        # the bases of every block on the chain's strands: exactly `score` equal pairs
        t, q, equal = head["tstart"], head["qstart"], 0
        for size, dt, dq in blocks:
            a = _side(case.seqs, head["tname"], "+", t, t + size)
            b = _side(case.seqs, head["qname"], head["qstrand"], q, q + size)
            assert len(a) == len(b) == size
            equal += sum(x == y for x, y in zip(a, b))
            t, q = t + size + dt, q + size + dq
        assert equal == head["score"] and (t, q) == (head["tend"], head["qend"])
    # the switch off again: the bytes of the run without it, no counts
    again, none, counts = _align([gpu], case, os.path.join(case.dir, "off.paf"), None)
    assert again == case.text and none is None and counts == (0, 0, 0, 0)


def test_driver_swapped(gpu, case):
    text, swapped, counts = _align([gpu], case, os.path.join(case.dir, "s.paf"), os.path.join(case.dir, "s.chain"), swap=True)
    records = _records_of(case.lines)
    assert text == case.text and swapped == M.chain_text(records, swap=True) and swapped != case.chain and counts == case.counts
    # the swapped file read as records of its own and swapped again with the model: the plain file
    back = []
    for head, blocks in M.parse_chains(swapped):
        runs = []
        for k, (size, dt, dq) in enumerate(blocks):
            runs += [(size, "=")] + ([(dt, "D")] if dt else []) + ([(dq, "I")] if dq else [])
        rev = head["qstrand"] == "-"
        back.append(dict(tname=head["tname"], tsize=head["tsize"], ts=head["tstart"], te=head["tend"], qname=head["qname"], qsize=head["qsize"], strand=head["qstrand"],
                         qs=head["qsize"] - head["qend"] if rev else head["qstart"], qe=head["qsize"] - head["qstart"] if rev else head["qend"], runs=runs))
    again = M.parse_chains(M.chain_text(back, swap=True))
    plain = M.parse_chains(case.chain)
    assert [(dict(h, score=0), b) for h, b in again] == [(dict(h, score=0), b) for h, b in plain]  # (the rebuilt runs have no X: the scores differ)


def test_driver_with_left_align(gpu, case):
    plain, _, _ = _align([gpu], case, os.path.join(case.dir, "la0.paf"), None, left=True)
    text, chain, counts = _align([gpu], case, os.path.join(case.dir, "la.paf"), os.path.join(case.dir, "la.chain"), left=True)
    assert text == plain != case.text
    want = M.chain_text(_records_of(text.decode().splitlines()))
    assert chain == want and counts == _counts_of(want)
    assert chain != case.chain  # the normalised runs are chained: a gap that moved moves a block's end


def test_driver_two_handles_on_one_device(gpu, case):
    h2 = capi.Handle(0)
    try:
        text, chain, counts = _align([gpu, h2], case, os.path.join(case.dir, "m.paf"), os.path.join(case.dir, "m.chain"))
    finally:
        h2.close()
    assert text == case.text and chain == case.chain and counts == case.counts


def test_driver_filtered_records_have_no_chain(gpu, case):
    text, chain, counts = _align([gpu], case, os.path.join(case.dir, "f.paf"), os.path.join(case.dir, "f.chain"), min_alignment_length=5000)
    lines = text.decode().splitlines()
    assert 0 < len(lines) < len(case.lines)
    want = M.chain_text(_records_of(lines))
    assert chain == want and counts == _counts_of(want) and counts[0] == len(lines)


def test_driver_two_gpus(gpu, case):
    if capi.load().wfm_device_count() < 2:
        pytest.skip("one GPU on this node: the two-GPU file cannot be made")
    h2 = capi.Handle(1)
    try:
        text, chain, counts = _align([gpu, h2], case, os.path.join(case.dir, "g2.paf"), os.path.join(case.dir, "g2.chain"))
    finally:
        h2.close()
    assert text == case.text and chain == case.chain and counts == case.counts


def test_chain_paf_entry_point(gpu, case):
    out = os.path.join(case.dir, "offline.chain")
    counts = capi.chain_paf(gpu, case.fa, os.path.join(case.dir, "plain.paf"), out)
    assert open(out, "rb").read() == case.chain and counts == case.counts
    counts = capi.chain_paf(gpu, case.fa, os.path.join(case.dir, "plain.paf"), out, swap=True)
    assert open(out, "rb").read() == M.chain_text(_records_of(case.lines), swap=True) and counts == case.counts


# ---- 3. the command line ----
def _cli(args, cwd=None):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "120", CLI] + args, capture_output=True, text=True, cwd=cwd)


def test_cli_beside_the_other_switches_and_from_the_paf(case):
    d = case.dir
    bed = os.path.join(d, "w.bed")
    with open(bed, "w") as f:
        for name, s in case.seqs.items():
            f.write("".join("%s\t%d\t%d\tw%d\n" % (name, a, min(len(s), a + 1000), a // 1000) for a in range(0, len(s), 1000)))
    files = {}
    for tag, extra in (("c0", []), ("c1", ["--chain", os.path.join(d, "c1.chain")])):
        out, lifted, bg = (os.path.join(d, "%s.%s" % (tag, ext)) for ext in ("paf", "lift", "bg"))
        r = _cli(["--lift", bed, "--lift-out", lifted, "--coverage", bg, "--cs", "-i", case.paf, "--out", out, case.fa] + extra)
        assert r.returncode == 0, r.stderr[-500:]
        files[tag] = [open(p, "rb").read() for p in (out, lifted, bg)]
        assert ("[wfmash::chain]" in r.stderr) == bool(extra)
    assert files["c0"] == files["c1"] and all(files["c0"])
    assert [l.rpartition("\tcs:Z:")[0] for l in files["c1"][0].decode().splitlines()] == case.lines
    assert open(os.path.join(d, "c1.chain"), "rb").read() == case.chain
    m = re.search(r"\[wfmash::chain\] (\d+) chains written, (\d+) blocks, (\d+) records refused", r.stderr)
    assert m and tuple(int(x) for x in m.groups()) == case.counts[:3]
    # the file again from the PAF the run wrote, swapped
    again = os.path.join(d, "c2.chain")
    r = _cli(["--chain-paf", os.path.join(d, "c1.paf"), "--chain", again, "--chain-swap", case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert open(again, "rb").read() == M.chain_text(_records_of(case.lines), swap=True)
    assert "%d chains written, %d blocks, 0 lines skipped" % case.counts[:2] in r.stderr
