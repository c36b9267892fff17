"""GPU tests of the net across records: wfm_net_* through capi, every piece and every record row held word for word against the brute
force of tests/net_model.py (one array cell per target base)."""
import os
import random
import re
import subprocess
import types

import numpy as np
import pytest

from tests import chain_model as CM
from tests import net_model as M
from tests import test_left_align_gpu as LT  # its synthetic pangenome (nothing of it is collected from here)
from tests.net_cases import HAND
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")

SPANS = capi.WFM_NET_SPANS
EQ = capi.WFM_NET_SCORE_EQ


# a problem is (order, score, base, [(op, length)])
def _add(net, problems, junk=0):
    """one wfm_net_add call; junk: unused words between the problems' runs"""
    probs, words = [], []
    for order, score, base, spec in problems:
        words += [0] * junk
        probs.append((base, len(words), len(spec), score, order))
        words += M.run_words(spec)
    return net.add(probs, words)


def _table(net):
    pieces, per = net.table()
    assert pieces.dtype.itemsize == 24 and per.dtype.itemsize == 48
    assert not per["zero"].any()
    return (list(zip(pieces["order"].tolist(), pieces["t"].tolist(), pieces["q"].tolist(), pieces["size"].tolist())),
            list(zip(per["order"].tolist(), per["score"].tolist(), per["first"].tolist(), per["count"].tolist(), per["bases_won"].tolist(),
                     per["bases_aligned"].tolist())))


def _model(problems, n_bases, lo=0):
    recs = [M.record(order, score, base, M.run_words(spec)) for order, score, base, spec in problems
            if not M.refused(base, M.run_words(spec), n_bases)]
    return M.net(recs, lo=lo)


def _fresh(gpu, problems, n_bases, calls=1, lo=0):
    """the table of a fresh object that got `problems` in `calls` add calls; held against the model"""
    net = gpu.net(n_bases)
    try:
        step = max(1, (len(problems) + calls - 1) // calls)
        for a in range(0, len(problems), step):
            flags = _add(net, problems[a:a + step])
            assert flags.tolist() == [SPANS if M.refused(b, M.run_words(s), n_bases) else 0 for _, _, b, s in problems[a:a + step]]
        got = _table(net)
        want = _model(problems, n_bases, lo)
        assert got[0] == want[0]
        assert got[1] == want[1]
        c = net.counts()
        assert c[0] == len(want[1]) and c[3] == len(want[0]) and c[4] == sum(1 for r in want[1] if r[3] == 0)
        return got
    finally:
        net.close()


@pytest.mark.parametrize("name,n_bases,problems,pieces,per", HAND, ids=[h[0] for h in HAND])
def test_hand_cases_word_for_word(gpu, name, n_bases, problems, pieces, per):
    got_pieces, got_per = _fresh(gpu, problems, n_bases)
    assert got_pieces == pieces
    assert [(r[1], r[3], r[4], r[5]) for r in got_per] == per


@pytest.mark.parametrize("n_blocks", [1, 255, 256, 257, 1025])
def test_blocks_of_one_problem_cross_the_round_carry(gpu, n_blocks):
    # block, gap, block, gap ...: 2 n - 1 runs, so the write kernel's rounds of 256 runs end inside a block, inside a gap and on either edge
    rng = random.Random(n_blocks)
    spec = []
    for k in range(n_blocks):
        if k:
            spec.append((rng.choice([M.OP_I, M.OP_D]), rng.randrange(1, 4)))
            if rng.random() < 0.3:
                spec.append((M.OP_D if spec[-1][0] == M.OP_I else M.OP_I, rng.randrange(1, 3)))
        spec.append((M.OP_M, rng.randrange(1, 5)))
        if rng.random() < 0.4:
            spec.append((M.OP_X, 1))
    span = sum(n for op, n in spec if op != M.OP_I)
    low = (1, 0, 3, [(M.OP_M, span)])  # a record under all of it: every gap of the first shows as a piece of the second
    pieces, per = _fresh(gpu, [(0, EQ, 3, spec), low], span + 10)
    assert per[0][3] == n_blocks and per[0][5] == per[0][4]


@pytest.mark.parametrize("m", [1, 2, 3, 1023, 1024, 1025])
def test_elementary_intervals_around_the_tree_and_scan_edges(gpu, m):
    # m elementary intervals: a staircase of m abutting blocks of changing owners, under one long block of the lowest record
    rng = random.Random(m)
    problems, t = [], 5
    for k in range(m):
        n = rng.randrange(1, 4)
        problems.append((k + 1, rng.randrange(1, 50), t, [(M.OP_M, n)]))
        t += n
    if m > 1:
        problems.append((0, 0, 5, [(M.OP_M, t - 5)]))
    net = gpu.net(t + 5)
    try:
        assert not _add(net, problems).any()
        got = _table(net)
        assert got == _model(problems, t + 5)
        assert net.counts()[2] == m
    finally:
        net.close()


@pytest.mark.parametrize("equal", [False, True], ids=["distinct_scores", "equal_scores"])
def test_pile_of_a_thousand_records(gpu, equal):
    rng = random.Random(7)
    scores = list(range(1000))
    rng.shuffle(scores)
    problems = [(10_000 - i, 5 if equal else scores[i], 100, [(M.OP_M, 64)]) for i in range(1000)]
    pieces, per = _fresh(gpu, problems, 300)
    best = min(p[0] for p in problems) if equal else problems[scores.index(999)][0]
    assert pieces == [(best, 100, 0, 64)]
    assert sum(1 for r in per if r[3] == 0) == 999


def test_nesting_ten_deep(gpu):
    # record k lies strictly inside record k - 1 and beats it: the outer ones are left with two flanks each
    problems = [(k, k, 100 + 7 * k, [(M.OP_M, 200 - 14 * k)]) for k in range(10)]
    pieces, per = _fresh(gpu, problems, 400)
    assert [r[3] for r in per] == [2] * 9 + [1]
    # and the other way round: the outermost wins everything
    pieces, per = _fresh(gpu, [(k, 100 - k, b, s) for k, _, b, s in problems], 400)
    assert pieces == [(0, 100, 0, 200)]


def test_coordinates_above_2_to_33(gpu):
    # only a list that follows the blocks can hold this: a cell per base would be 2^34 cells
    far = (1 << 33) + 12345
    n_bases = 1 << 34
    problems = [(0, 5, far, [(M.OP_M, 40), (M.OP_D, 10), (M.OP_M, 40)]), (1, 9, far + 30, [(M.OP_I, 7), (M.OP_M, 30)]),
                (2, 1, n_bases - 20, [(M.OP_M, 20)]), (3, 2, 0, [(M.OP_M, 3)])]
    net = gpu.net(n_bases)
    try:
        assert not _add(net, problems).any()
        got = _table(net)
        # the model's cells cover a window: the two far records there, the other two alone in theirs
        near = _model(problems[:2], n_bases, lo=far - 5)
        last = _model(problems[2:3], n_bases, lo=n_bases - 30)
        first = _model(problems[3:], n_bases)
        assert got[0] == near[0] + last[0] + first[0]
        assert [r[:2] + r[3:] for r in got[1]] == [r[:2] + r[3:] for r in near[1] + last[1] + first[1]]
    finally:
        net.close()
    with pytest.raises(capi.WfmError):
        gpu.net(1 << 40)


def _fuzz(seed, n_problems=60, depth=8):
    """problems whose blocks pile up to `depth` deep: every `depth` of them share a window of 1200 bases, which a problem (at most 11 runs
    of fewer than 90 bases from one of its first 200) cannot leave"""
    rng = random.Random(seed)
    problems = []
    n_bases = 1200 * ((n_problems + depth - 1) // depth) + 17
    for i in range(n_problems):
        base = 1200 * (i // depth) + rng.randrange(0, 200)
        spec = []
        for _ in range(rng.randrange(1, 12)):
            op = rng.choice([M.OP_M, M.OP_M, M.OP_X, M.OP_I, M.OP_D])
            if spec and spec[-1][0] == op:
                continue
            spec.append((op, rng.randrange(1, 90 if op <= M.OP_X else 25)))
        score = rng.choice([EQ, EQ, rng.randrange(0, 4), rng.randrange(0, 300)])
        problems.append((rng.randrange(0, 1 << 40) * 64 + i, score, base, spec))
    return problems, n_bases


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_fuzz_against_the_model(gpu, seed):
    problems, n_bases = _fuzz(seed)
    pieces, per = _fresh(gpu, problems, n_bases)
    assert len(per) == 60 and max(r[3] for r in per) >= 2


def test_order_and_split_of_the_calls_change_nothing(gpu):
    problems, n_bases = _fuzz(21)
    want = _fresh(gpu, problems, n_bases)
    shuffled = list(problems)
    random.Random(5).shuffle(shuffled)
    for calls in (1, 2, 7):
        assert _fresh(gpu, shuffled, n_bases, calls=calls) == want
        assert _fresh(gpu, problems, n_bases, calls=calls) == want


def test_export_import_merges_objects(gpu):
    problems, n_bases = _fuzz(31)
    want = _fresh(gpu, problems, n_bases)
    a, b, c = gpu.net(n_bases), gpu.net(n_bases), gpu.net(n_bases)
    try:
        _add(a, problems[:25]); _add(b, problems[25:])
        for src in (b, a):
            blocks, recs = src.export()
            assert blocks.dtype.itemsize == 24 and recs.dtype.itemsize == 16
            c.import_(blocks, recs)
        assert _table(c) == want
        assert c.counts()[:2] == (a.counts()[0] + b.counts()[0], a.counts()[1] + b.counts()[1])
        # the export of an empty object, and the import of nothing
        e = gpu.net(n_bases)
        blocks, recs = e.export()
        assert len(blocks) == 0 and len(recs) == 0
        c.import_(blocks, recs)
        assert _table(c) == want
        e.close()
    finally:
        a.close(); b.close(); c.close()


def test_small_output_chunks_and_two_calls_give_the_same_bytes(gpu, monkeypatch):
    problems, n_bases = _fuzz(41)
    net = gpu.net(n_bases)
    try:
        _add(net, problems)
        p0, r0 = net.table()
        p1, r1 = net.table()
        assert p0.tobytes() == p1.tobytes() and r0.tobytes() == r1.tobytes() and len(p0) > 40
        monkeypatch.setenv("WFM_NET_OUT_MB", repr(300 / 1048576.0))  # 12 pieces a chunk
        p2, r2 = net.table()
        monkeypatch.setenv("WFM_NET_OUT_MB", "0")                    # one piece a chunk
        p3, r3 = net.table()
        assert p2.tobytes() == p0.tobytes() and r2.tobytes() == r0.tobytes()
        assert p3.tobytes() == p0.tobytes() and r3.tobytes() == r0.tobytes()
    finally:
        net.close()


def test_flagged_problem_between_good_ones(gpu):
    good = [(0, 5, 10, [(M.OP_M, 20)]), (1, 9, 15, [(M.OP_M, 10), (M.OP_D, 3), (M.OP_X, 4)])]
    bad = [(7, 99, 10, [(M.OP_M, 4), (M.OP_X, 0), (M.OP_M, 4)]),   # an empty run
           (8, 99, 10, []),                                        # no runs
           (9, 99, 90, [(M.OP_M, 11)]),                            # leaves the target
           (10, 99, 101, [(M.OP_I, 1)])]                           # begins behind it
    for b in bad:
        problems = [good[0], b, good[1]]
        net = gpu.net(100)
        try:
            assert _add(net, problems, junk=3).tolist() == [0, SPANS, 0]
            assert _table(net) == _model(good, 100)
            assert net.counts()[:2] == (2, 3)
        finally:
            net.close()


def test_refusals_leave_the_object_and_the_handle_usable(gpu):
    problems = [(0, 5, 10, [(M.OP_M, 20)]), (1, 9, 15, [(M.OP_M, 10)])]
    net = gpu.net(100)
    try:
        _add(net, problems)
        want = _table(net)
        # a run range past the buffer: nothing is added
        with pytest.raises(capi.WfmError, match="leave the run buffer"):
            net.add([(0, 0, 1, 3, 5), (0, 1, 2, 3, 6)], M.run_words([(M.OP_M, 4), (M.OP_M, 4)]))
        assert _table(net) == want
        # bad imports: an empty block, one that leaves the target, one whose record is nowhere; nothing is added
        rec = np.array([(50, 3, 0)], dtype=capi.NET_REC_DTYPE)
        for blk in [(50, 5, 0, 0), (50, 95, 0, 6), (51, 5, 0, 2), (50, 5, 0xfffffffe, 2)]:
            with pytest.raises(capi.WfmError, match="nothing was added"):
                net.import_(np.array([blk], dtype=capi.NET_BLOCK_DTYPE), rec)
        assert net.counts()[:2] == (2, 2) and _table(net) == want
        # a block of a record the object already has is fine
        net.import_(np.array([(1, 60, 0, 5)], dtype=capi.NET_BLOCK_DTYPE), np.zeros(0, dtype=capi.NET_REC_DTYPE))
        assert _table(net)[0] == want[0] + [(1, 60, 0, 5)]
        # a duplicate order: the table refuses, and goes on refusing, while the handle works on
        _add(net, [(1, 2, 70, [(M.OP_M, 5)])])
        for _ in range(2):
            with pytest.raises(capi.WfmError, match="same order"):
                net.table()
        other = gpu.net(100)
        _add(other, problems)
        assert _table(other) == want
        other.close()
    finally:
        net.close()


def test_empty_object(gpu):
    net = gpu.net(1000)
    try:
        pieces, per = net.table()
        assert len(pieces) == 0 and len(per) == 0
        assert net.add([], []).tolist() == []
        assert net.counts() == (0, 0, 0, 0, 0)
        # records without blocks alone: rows, and no pieces
        _add(net, [(4, 1, 10, [(M.OP_D, 5)]), (2, EQ, 10, [(M.OP_I, 5)])])
        assert _table(net) == ([], [(2, 0, 0, 0, 0, 0), (4, 1, 0, 0, 0, 0)])
    finally:
        net.close()


def test_table_then_more_adds_then_table(gpu):
    problems, n_bases = _fuzz(51)
    net = gpu.net(n_bases)
    try:
        _add(net, problems[:20])
        assert _table(net) == _model(problems[:20], n_bases)
        _add(net, problems[20:45]); _add(net, problems[45:])
        assert _table(net) == _fresh(gpu, problems, n_bases)
    finally:
        net.close()


def test_interleaved_with_chain_runs_and_a_pav_on_one_handle(gpu):
    problems, n_bases = _fuzz(61, n_problems=24)
    net, pav = gpu.net(n_bases), gpu.pav(n_bases, 2)
    try:
        for a in range(0, 24, 8):
            part = problems[a:a + 8]
            _add(net, part)
            probs, words = [], []
            for order, score, base, spec in part:
                probs.append((len(words), len(spec), 0))
                words += M.run_words(spec)
            blocks, per = gpu.chain_runs(probs, words)
            # the chain's blocks are the net's: the same stretches, in the same order
            want = [n for _, _, base, spec in part for (_, _, n) in M.blocks_of_runs(base, M.run_words(spec))[0]]
            assert blocks["size"].tolist() == want
            pav.add([(base, off, n, 0) for (off, n, _), (_, _, base, _) in zip(probs, part)], words)
            pav.union()
        assert _table(net) == _model(problems, n_bases)
        won = sum(r[4] for r in _table(net)[1])
        assert won == int(pav.matrix([(0, n_bases)])[0][0])  # every aligned base has exactly one owner
    finally:
        net.close(); pav.close()


# ---- the align driver, on the synthetic pangenome tests/test_chain_gpu.py borrows from tests/test_left_align_gpu.py ----
def _align(handles, case, out, net, chain=None, left=False, **params):
    capi.set_chain_net(net)
    capi.set_chain(chain, False)
    capi.set_left_align(left)
    try:
        if len(handles) == 1:
            capi.align_paf(handles[0], case.fa, case.paf, out, params=params or None)
        else:
            capi.align_paf_multi(handles, case.fa, case.paf, out, params=params or None)
        return (open(out, "rb").read(), open(net, "rb").read() if net else None, open(chain, "rb").read() if chain else None,
                capi.chain_net_counts())
    finally:
        capi.set_chain_net(None)
        capi.set_chain(None)
        capi.set_left_align(False)


def _fasta_offsets(path):
    """where every sequence of the FASTA begins in the concatenation, in file order"""
    off, at, name = {}, 0, None
    for line in open(path):
        if line.startswith(">"):
            name = line[1:].split()[0]
            off[name] = at
        else:
            at += len(line.strip())
    return off, at


def _records_of(paf_lines, offsets):
    out = []
    for line in paf_lines:
        f = line.rstrip("\n").split("\t")
        cg = [v for v in f[12:] if v.startswith("cg:Z:")][0][5:]
        out.append(dict(qname=f[0], qsize=int(f[1]), qs=int(f[2]), qe=int(f[3]), strand=f[4], tname=f[5], tsize=int(f[6]), ts=int(f[7]), te=int(f[8]),
                        runs=[(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cg)], t_offset=offsets[f[5]]))
    return out


def _counts_of(text, n_records):
    chains = CM.parse_chains(text)
    return (n_records, len(chains), sum(len(b) for _, b in chains), n_records - len(chains))


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows, the files of a run with --chain alone and of one with --chain and --chain-net: made once, never
    changed"""
    d = str(tmp_path_factory.mktemp("chain_net"))
    fa, paf, seqs = LT._make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, seqs=seqs)
    c.offsets, c.n_bases = _fasta_offsets(fa)
    c.text, none, c.chain, counts = _align([gpu], c, os.path.join(d, "plain.paf"), None, chain=os.path.join(d, "plain.chain"))
    assert none is None and counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20
    c.with_text, c.net, c.with_chain, c.counts = _align([gpu], c, os.path.join(d, "with.paf"), os.path.join(d, "with.net.chain"),
                                                        chain=os.path.join(d, "with.chain"))
    return c


def test_driver_changes_no_byte_of_the_paf_or_the_chain_file(gpu, case):
    assert case.with_text == case.text and case.with_chain == case.chain
    text, net, none, counts = _align([gpu], case, os.path.join(case.dir, "alone.paf"), os.path.join(case.dir, "alone.net.chain"))
    assert text == case.text and net == case.net and none is None and counts == case.counts  # without --chain: the same net file


def test_driver_file_is_the_models(gpu, case):
    want = _model_text(case)
    assert case.net == want
    assert case.counts == _counts_of(want, len(case.lines))
    chains = CM.parse_chains(case.net)
    assert [h["id"] for h, _ in chains] == list(range(1, len(chains) + 1)) and 0 < len(chains) <= len(case.lines)
    assert any(dt and dq for _, blocks in chains for _, dt, dq in blocks)  # a record cut by another: both distances are non-zero
    # the header's score is the score the record competed with: the = columns, which the plain file has for the same record
    plain = {}
    for h, _ in CM.parse_chains(case.chain):
        plain.setdefault((h["qname"], h["qstrand"], h["tname"]), set()).add(h["score"])
    assert all(h["score"] in plain[(h["qname"], h["qstrand"], h["tname"])] for h, _ in chains)


def _model_text(case, lines=None):
    return M.chain_text(_records_of(case.lines if lines is None else lines, case.offsets), case.n_bases)


def _paint(text, name, size):
    """per base of the first side `name`: [(score, id, qname, qstrand, forward position on the second side)], chain_model.lift_pos's rule"""
    cells = [[] for _ in range(size)]
    for head, blocks in CM.parse_chains(text):
        if head["tname"] != name:
            continue
        t, q = head["tstart"], head["qstart"]
        for n, dt, dq in blocks:
            for k in range(n):
                at = q + k
                cells[t + k].append((head["score"], head["id"], head["qname"], head["qstrand"], head["qsize"] - 1 - at if head["qstrand"] == "-" else at))
            t, q = t + n + dt, q + n + dq
    return cells


def test_driver_every_target_base_lifts_once_and_to_the_best_chain(gpu, case):
    name = max(case.offsets, key=lambda k: sum(1 for ln in case.lines if ln.split("\t")[5] == k))  # the sequence most records lie on
    size = len(case.seqs[name])
    net, plain = _paint(case.net, name, size), _paint(case.chain, name, size)
    assert max(len(c) for c in plain) >= 2  # the plain file is NOT single coverage here: there is something to decide
    for pos in range(size):
        assert len(net[pos]) <= 1
        assert bool(net[pos]) == bool(plain[pos])
        if plain[pos]:
            best = max(plain[pos], key=lambda h: (h[0], -h[1]))
            assert net[pos][0][2:] == best[2:] and net[pos][0][0] == best[0]
    for pos in range(0, size, 97):  # the painting is chain_model.lift_pos's rule
        assert [h[2:] for h in net[pos]] == CM.lift_pos(case.net, name, pos)
        assert sorted(h[2:] for h in plain[pos]) == sorted(CM.lift_pos(case.chain, name, pos))


def test_driver_with_left_align(gpu, case):
    text, net, chain, counts = _align([gpu], case, os.path.join(case.dir, "la.paf"), os.path.join(case.dir, "la.net.chain"),
                                      chain=os.path.join(case.dir, "la.chain"), left=True)
    assert text != case.text
    lines = text.decode().splitlines()
    want = _model_text(case, lines)
    assert net == want and counts == _counts_of(want, len(lines))
    assert chain == CM.chain_text(_records_of(lines, case.offsets))
    assert net != case.net  # the normalised runs compete: a gap that moved moves a piece's end


def test_driver_two_handles_on_one_device(gpu, case):
    h2 = capi.Handle(0)
    try:
        text, net, chain, counts = _align([gpu, h2], case, os.path.join(case.dir, "m.paf"), os.path.join(case.dir, "m.net.chain"),
                                          chain=os.path.join(case.dir, "m.chain"))
    finally:
        h2.close()
    assert text == case.text and net == case.net and chain == case.chain and counts == case.counts


def test_driver_two_gpus(gpu, case):
    if capi.load().wfm_device_count() < 2:
        pytest.skip("one GPU on this node: the two-GPU file cannot be made")
    h2 = capi.Handle(1)
    try:
        text, net, chain, counts = _align([gpu, h2], case, os.path.join(case.dir, "g2.paf"), os.path.join(case.dir, "g2.net.chain"))
    finally:
        h2.close()
    assert text == case.text and net == case.net and counts == case.counts


def test_driver_filtered_records_have_no_chain(gpu, case):
    text, net, _, counts = _align([gpu], case, os.path.join(case.dir, "f.paf"), os.path.join(case.dir, "f.net.chain"), min_alignment_length=5000)
    lines = text.decode().splitlines()
    assert 0 < len(lines) < len(case.lines)
    want = _model_text(case, lines)
    assert net == want and counts == _counts_of(want, len(lines)) and net != case.net  # a record that is gone competes no more


def test_chain_paf_entry_point(gpu, case):
    out, net = os.path.join(case.dir, "offline.chain"), os.path.join(case.dir, "offline.net.chain")
    counts = capi.chain_paf(gpu, case.fa, os.path.join(case.dir, "plain.paf"), None, net_path=net)
    assert open(net, "rb").read() == case.net and counts == case.counts
    counts = capi.chain_paf(gpu, case.fa, os.path.join(case.dir, "plain.paf"), out, net_path=net)
    assert open(net, "rb").read() == case.net and open(out, "rb").read() == case.chain and counts == _chain_counts_of(case.chain)


def _chain_counts_of(text):
    chains = CM.parse_chains(text)
    return (len(chains), sum(len(b) for _, b in chains), 0, 0)


def _cli(args, cwd=None):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "120", CLI] + args, capture_output=True, text=True, cwd=cwd)


def test_cli_files_and_refusals(case):
    d = case.dir
    out, net, chain = (os.path.join(d, "cli." + ext) for ext in ("paf", "net.chain", "chain"))
    r = _cli(["--chain-net", net, "--chain", chain, "-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert open(out, "rb").read() == case.text and open(net, "rb").read() == case.net and open(chain, "rb").read() == case.chain
    m = re.search(r"\[wfmash::chain-net\] (\d+) records added, (\d+) chains written, (\d+) pieces, (\d+) records won nothing", r.stderr)
    assert m and tuple(int(x) for x in m.groups()) == case.counts
    # the file again from the PAF the run wrote, without --chain
    again = os.path.join(d, "cli2.net.chain")
    r = _cli(["--chain-paf", out, "--chain-net", again, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert open(again, "rb").read() == case.net
    # the refusals: usage errors that name the reason, and no file
    gone = os.path.join(d, "refused.net.chain")
    for extra, why in ((["-m"], "cannot be combined with -m"), (["--verify-paf", out], "cannot be combined with --verify-paf"),
                       (["--chain", chain, "--chain-swap"], "nets on the query side are not done"), (["--chain-swap"], "nets on the query side are not done")):
        r = _cli(["--chain-net", gone] + extra + [case.fa])
        assert r.returncode == 1 and "--chain-net" in r.stderr and why in r.stderr, (extra, r.stderr[-300:])
        assert not os.path.exists(gone)
