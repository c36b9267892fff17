"""CPU tests: the WFA oracle (oracle/wfa2p.c) against an independent O(nm) DP.

The reference holds no golden vector at the WFA2-lib boundary (SURVEY.md 8c:
"parity unpinned"), so the oracle is pinned by (i) optimal score == 5-state DP,
(ii) pafcheck-style CIGAR validity, (iii) CIGAR-implied score == optimal score.
"""
import random

import pytest

import endsfree_cases
from wfmash_amd import synth


def _rand_pairs(seed, n, lens, rates):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = rng.choice(lens)
        p = synth.random_dna(seed * 1000 + i, L)
        t = synth.mutate(p, rng.choice(rates), seed * 7919 + i) if L else b""
        if rng.random() < 0.15:
            t = synth.random_dna(seed * 31 + i, rng.randrange(0, 200))
        out.append((p, t))
    return out


def test_uni_and_biwfa_scores_match_dp(oracle):
    for p, t in _rand_pairs(11, 120, [0, 1, 2, 7, 40, 100, 101, 160, 420, 900], [0.0, 0.02, 0.1, 0.3]):
        dp = oracle.dp_score(p, t)
        rc, ops, sc, _ = oracle.align_uni(p, t)
        assert rc == 0 and sc == dp
        assert oracle.ops_check(ops, p, t) == 0
        assert oracle.ops_score(ops) == dp
        rc, ops2, sc2, _ = oracle.align_biwfa(p, t)
        assert rc == 0 and sc2 == dp
        assert oracle.ops_check(ops2, p, t) == 0


def test_biwfa_recursion_is_exercised(oracle):
    p = synth.random_dna(5, 6000)
    t = synth.mutate(p, 0.1, 55)
    rc, ops, sc, st = oracle.align_biwfa(p, t)
    assert rc == 0
    assert st.bialign_calls >= 3 and st.base_calls >= 4 and st.max_depth >= 2
    assert sc == oracle.dp_score(p, t)
    assert oracle.ops_check(ops, p, t) == 0


def test_endsfree_scores_match_dp(oracle):
    rng = random.Random(3)
    for i in range(80):
        p = synth.random_dna(300 + i, rng.choice([1, 20, 150, 400]))
        t = synth.mutate(p, rng.choice([0.0, 0.05, 0.2]), 900 + i)
        if rng.random() < 0.4:
            t = synth.random_dna(77 + i, rng.randrange(1, 40)) + t
        if rng.random() < 0.4:
            p = synth.random_dna(99 + i, rng.randrange(1, 40)) + p
        if not t:
            continue
        for args in ((len(p), 0, len(t), 0), (0, len(p), 0, len(t))):  # head / tail patch forms (wflign.cpp:300-305, 392-397)
            dp = oracle.dp_score_endsfree(p, t, *args)
            rc, ops, sc, _ = oracle.align_endsfree(p, args[0], args[1], t, args[2], args[3])
            assert rc == 0 and sc == dp
            assert oracle.ops_check(ops, p, t) == 0


@pytest.mark.parametrize("pen", endsfree_cases.PENS, ids=lambda p: "default" if p is None else "-".join(map(str, p)))
def test_endsfree_general_free_lengths_match_dp(oracle, pen):
    """The four free lengths as independent values (tests/endsfree_cases.py: partial lengths, one free end alone, begin and end free at
    once, empty sides): the oracle's score is the O(nm) DP's, its op string spans both sequences, and the string priced on its own
    (endsfree_price: no code of the oracle's) costs exactly that score.  Every case is asserted."""
    cases = endsfree_cases.build_cases()
    assert len(cases) >= 350
    some_gap_free = 0
    for c in cases:
        dp = oracle.dp_score_endsfree(c.p, c.t, *c.free, pen=pen)
        rc, ops, sc, _ = oracle.align_endsfree(c.p, c.free[0], c.free[1], c.t, c.free[2], c.free[3], pen=pen)
        assert rc == 0, (c.name, c.free)
        assert sc == dp, (c.name, c.free, sc, dp)
        assert oracle.ops_check(ops, c.p, c.t) == 0, (c.name, c.free)
        assert endsfree_cases.endsfree_price(ops, c.free, pen) == sc, (c.name, c.free, sc)
        some_gap_free += oracle.ops_score(ops, pen) != sc
    assert some_gap_free * 3 >= len(cases)  # (the family is about free gaps: a third of it at least uses one)


def test_endsfree_price_on_hand_made_strings():
    price = endsfree_cases.endsfree_price
    assert price(b"IIIIIIIIII", (0, 0, 4, 3)) == 8 + 2 * 3  # one run: both allowances of its side
    assert price(b"IIIIIIIIII", (0, 0, 10, 0)) == 0 and price(b"IIIIIIIIII", (0, 0, 6, 6)) == 0
    assert price(b"IIIIIIIIII", (4, 3, 0, 0)) == 8 + 2 * 10  # (the pattern's allowances do not free text bases)
    assert price(b"DDDMMXMMII", (2, 0, 9, 1)) == (8 + 2 * 1) + 5 + (8 + 2 * 1)
    assert price(b"DDDIII", (3, 0, 0, 3)) == 0 and price(b"DDDIII", (0, 3, 3, 0)) == 2 * (8 + 2 * 3)  # begin-free I behind a D: not leading
    assert price(b"MMIDMM", (9, 9, 9, 9)) == 2 * (8 + 2)  # gaps inside are paid
    assert price(b"D" * 40 + b"M", (10, 0, 0, 0)) == 24 + 30 and price(b"", (1, 1, 1, 1)) == 0
    assert price(b"XDD", (0, 1, 0, 0), (4, 6, 2, 12, 1)) == 4 + 6 + 2


def test_component_halves_concatenate(oracle):
    """A BiWFA breakpoint splits the problem into two halves whose component-
    constrained alignments concatenate to an optimal alignment."""
    p = synth.random_dna(8, 3000)
    t = synth.mutate(p, 0.08, 88)
    rc, bp, _ = oracle.find_breakpoint(p, t)
    assert rc == 0
    dp = oracle.dp_score(p, t)
    assert bp.score == dp
    h, v = bp.offset_forward, bp.offset_forward - bp.k_forward
    rc0, ops0, _, _ = oracle.align_comp(p[:v], t[:h], 0, bp.component)
    rc1, ops1, _, _ = oracle.align_comp(p[v:], t[h:], bp.component, 0)
    assert rc0 == 0 and rc1 == 0
    ops = ops0 + ops1
    assert oracle.ops_check(ops, p, t) == 0
    assert oracle.ops_score(ops) == dp


def test_custom_penalties(oracle):
    pen = (4, 6, 2, 12, 1)
    for p, t in _rand_pairs(21, 30, [50, 300, 700], [0.05, 0.2]):
        rc, ops, sc, _ = oracle.align_biwfa(p, t, pen)
        assert rc == 0 and sc == oracle.dp_score(p, t, pen)


def test_legacy_reads_fixture_is_plausible(oracle):
    """test/data/regression/reads.255bps.paf predates the current writer (its
    CIGARs start/end with indels); it cannot be a byte-exact golden, but the
    alignment score of our oracle must not be worse than the legacy CIGAR's."""
    import gzip
    import os
    here = os.path.dirname(__file__)
    fa = os.path.join(here, "golden", "reads.255bps.fa.gz")
    paf = os.path.join(here, "golden", "reads.255bps.paf")
    if not (os.path.exists(fa) and os.path.exists(paf)):
        pytest.skip("fixture not present")
    seqs = {}
    name = None
    for line in gzip.open(fa, "rt"):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = ""
        elif name:
            seqs[name] += line.upper()
    import re
    n = 0
    for line in open(paf):
        f = line.rstrip("\n").split("\t")
        q, qs, qe, strand, tname, ts, te = f[0], int(f[2]), int(f[3]), f[4], f[5], int(f[7]), int(f[8])
        cg = [x for x in f if x.startswith("cg:Z:")][0][5:]
        if strand != "+":
            continue
        query = seqs[q][qs:qe].encode()
        target = seqs[tname][ts:te].encode()
        legacy_ops = b"".join((b"M" if op in "=M" else op.encode()) * int(cnt) for cnt, op in re.findall(r"(\d+)([=XIDM])", cg))
        # legacy "M"/"=" may hide mismatches: re-derive X from the sequences
        v = h = 0
        fixed = bytearray()
        for op in legacy_ops:
            c = chr(op)
            if c == "M":
                fixed.append(ord("M") if target[v] == query[h] else ord("X"))
                v += 1
                h += 1
            elif c == "X":
                fixed.append(op)
                v += 1
                h += 1
            elif c == "I":
                fixed.append(op)
                h += 1
            else:
                fixed.append(op)
                v += 1
        assert v == len(target) and h == len(query)
        rc, ops, sc, _ = oracle.align_biwfa(target, query)
        assert rc == 0 and sc <= oracle.ops_score(bytes(fixed))
        n += 1
    assert n >= 1


def test_a_score_bound_does_not_change_the_breakpoint(oracle):
    """The product cuts its wavefronts to the diagonals from which the end is within reach of a score bound (children of a
    BiWFA split: the score their parent found + two gap openings; roots: the caller's guess) and starts the overlap loop
    as if a breakpoint just above the bound were in hand.  The claim -- same breakpoint, field for field, whenever the
    bound holds; nothing found when it does not -- is checked here on the CPU restatement of the reference's loop, with
    the cut and the stand-in added to it (oracle/wfa2p.c: wfo_find_breakpoint_bounded), over padded records, structural
    differences, and begin / end components as the recursion produces them."""
    rng = random.Random(77)
    fields = ("score", "score_forward", "score_reverse", "k_forward", "k_reverse", "offset_forward", "offset_reverse", "component")
    checked = failed_as_expected = fewer_cells = 0
    for i in range(260):
        L = rng.choice([300, 900, 2500])
        core = synth.random_dna(9000 + i, L)
        q = synth.mutate(core, rng.choice([0.002, 0.02, 0.08]), 31 * i + 1)
        shape = i % 4
        if shape == 0:      # a query against its padded window: two end gaps
            tgt = synth.random_dna(50000 + i, rng.randrange(20, 400)) + core + synth.random_dna(60000 + i, rng.randrange(20, 400))
        elif shape == 1:    # one-sided padding
            tgt = core + synth.random_dna(60000 + i, rng.randrange(50, 600))
        elif shape == 2:    # a structural difference in the middle
            cut = rng.randrange(50, 300)
            tgt, q = core, q[:len(q) // 2] + q[len(q) // 2 + cut:]
        else:               # balanced
            tgt = core
        constrained = i % 3 == 0
        cb, ce = (rng.randrange(0, 5), rng.randrange(0, 5)) if constrained else (0, 0)
        rc0, bp0, st0 = oracle.find_breakpoint(tgt, q, cb, ce)
        if rc0 != 0:
            continue
        S = bp0.score
        slack = 2 * 24 + 8 if constrained else 0  # a child that begins or ends inside a gap: see wfa_host.hip (children's bounds)
        for sub in (S + slack, S + slack + 1, S + slack + 9, S + 300, 3 * S + 1000):
            rc, bp, st = oracle.find_breakpoint_bounded(tgt, q, sub, cb, ce)
            assert rc == 0, (i, shape, cb, ce, S, sub, rc)
            assert all(getattr(bp, f) == getattr(bp0, f) for f in fields), (i, shape, cb, ce, S, sub)
            assert st.cells <= st0.cells
            fewer_cells += st.cells < st0.cells
            checked += 1
        for sub in (S - 1, S // 2):
            if sub < 1:
                continue
            rc, bp, st = oracle.find_breakpoint_bounded(tgt, q, sub, cb, ce)
            assert rc != 0, (i, shape, cb, ce, S, sub, bp.score)
            failed_as_expected += 1
    assert checked > 700 and failed_as_expected > 250 and fewer_cells > 200, (checked, failed_as_expected, fewer_cells)


def test_cutting_the_overlap_loop_into_rounds_does_not_change_the_breakpoint(oracle):
    """The product's phase 2 runs in rounds of 2 x 32 tests: a job whose loop has not ended takes another round from the state it
    is in, the breakpoint so far set aside and its score handed on as if it were a bound (BpJob::best0); a round that ends the loop
    without a better one reports WFM_DEV_P2_NOTHING and the one set aside stands.  The protocol on the CPU restatement of the
    reference's loop (oracle/wfa2p.c: wfo_find_breakpoint_rounds): the same breakpoint, field for field, for any round length, with
    and without a score bound -- on records whose loop is long (unrelated sequences, moved blocks: the antidiagonals touch long
    before two cells share a diagonal) as well as ordinary ones."""
    rng = random.Random(41)
    fields = ("score", "score_forward", "score_reverse", "k_forward", "k_reverse", "offset_forward", "offset_reverse", "component")
    multi = checked = 0
    for i in range(120):
        shape = i % 4
        if shape == 0:    # unrelated
            a, b = synth.random_dna(100 + i, rng.choice([300, 700])), synth.random_dna(300 + i, rng.choice([250, 800]))
        elif shape == 1:  # a block moved to the end
            u, v, w = synth.random_dna(500 + i, 300), synth.random_dna(700 + i, 200), synth.random_dna(900 + i, 300)
            a, b = u + v + w, u + w + synth.mutate(v, 0.03, i)
        elif shape == 2:  # ordinary divergence
            a = synth.random_dna(1100 + i, 900)
            b = synth.mutate(a, rng.choice([0.02, 0.1]), 7 * i)
        else:             # padded window
            b = synth.random_dna(1300 + i, 600)
            a = synth.random_dna(1500 + i, 150) + synth.mutate(b, 0.01, 3 * i) + synth.random_dna(1700 + i, 90)
        cb, ce = (rng.randrange(0, 5), rng.randrange(0, 5)) if i % 5 == 0 else (0, 0)
        rc0, bp0, _ = oracle.find_breakpoint(a, b, cb, ce)
        if rc0 != 0:
            continue
        for per_round in (1, 2, 5, 16, 64):
            for sub in (-1, bp0.score + 2 * 24 + 8 + rng.randrange(0, 50)):
                rc, bp, rounds = oracle.find_breakpoint_rounds(a, b, per_round, sub, cb, ce)
                assert rc == 0, (i, shape, per_round, sub, rc)
                assert all(getattr(bp, f) == getattr(bp0, f) for f in fields), (i, shape, per_round, sub, rounds)
                multi += rounds > 1
                checked += 1
    assert checked > 900 and multi > 600, (checked, multi)


# ---- the meeting point of the two directions (wfo_meet_point): what the product's tile phase replays block by block


def _with_subs(p, K):
    a = bytearray(p)
    for i in range(K):
        pos = (2 * i + 1) * len(p) // (2 * K)
        a[pos:pos + 1] = a[pos:pos + 1].translate(bytes.maketrans(b"ACGT", b"CGTA"))
    return bytes(a)


def test_meet_point_of_evenly_spaced_substitutions(oracle):
    """K evenly spaced substitutions in 4000 bases, default penalties: each direction pays 5 per substitution it passes, the forward
    one steps first, and the loop ends when the two have paid all K between them -- sf = 5 ceil(K / 2), sr = sf - (K odd)."""
    p = synth.random_dna(0x3E37, 4000)
    assert oracle.meet_point(p, _with_subs(p, 41)) == (105, 104, 1)
    assert oracle.meet_point(p, _with_subs(p, 42)) == (105, 105, 0)
    for K in range(1, 170):
        sf = 5 * ((K + 1) // 2)
        assert oracle.meet_point(p, _with_subs(p, K)) == (sf, sf - K % 2, K % 2), K
    assert oracle.meet_point(p, p) == (0, 0, 0)  # met before the first step


def test_meet_point_against_the_breakpoint(oracle):
    """Any penalties, any begin / end components: sf - sr is 0 or 1, and 1 exactly when the forward step was the last.  The
    breakpoint is found by the second loop, which goes on from the meeting point: every overlap test pairs the wavefront of the
    step at hand (a score >= the meeting point's) with wavefronts of the other direction up to scope - 1 scores behind ITS step
    -- so one of the breakpoint's two scores is at or beyond the meeting point and the other less than a scope short of it."""
    rng = random.Random(5)
    n = 0
    for i in range(200):
        L = rng.choice([130, 300, 700, 1500])
        p = synth.random_dna(1000 + i, L)
        t = synth.mutate(p, rng.choice([0.01, 0.05, 0.15, 0.3]), 77 + i)
        pen = rng.choice([None, (4, 6, 2, 12, 1), (3, 4, 2, 24, 1)])
        cb, ce = rng.choice([(0, 0), (0, 0), (1, 0), (0, 3), (2, 4), (4, 1)])
        sf, sr, last_fwd = oracle.meet_point(p, t, pen, cb, ce)
        assert sf - sr in (0, 1) and sf - sr == last_fwd
        rc, bp, _ = oracle.find_breakpoint(p, t, cb, ce, pen)
        if rc != 0:
            assert (sf, sr) == (0, 0)
            continue
        n += 1
        x, o1, e1, o2, e2 = pen or oracle.DEFAULT_PEN
        scope = max(x, o1 + e1, o2 + e2) + 1
        assert (bp.score_forward >= sf and bp.score_reverse > sr - scope) or (bp.score_reverse >= sr and bp.score_forward > sf - scope), \
            (sf, sr, bp.score_forward, bp.score_reverse)
    assert n >= 180


def _all_rows(oracle, p, t, upto, **kw):
    """{(component, score): {k: offset}} of forward_rows for every score 0 .. upto, from calls 26 scores apart (one pass)"""
    scores = sorted(set(range(upto, -1, -oracle.ROWS)))
    kmin, off, rng = oracle.forward_rows(p, t, scores, **kw)
    out = {}
    for i, s in enumerate(scores):
        for c in range(5):
            for back in range(oracle.ROWS):
                if s - back < 0:
                    assert rng[i, c, back, 0] > rng[i, c, back, 1] and (off[i, c, back] == oracle.ROW_NULL).all()
                    continue
                lo, hi = int(rng[i, c, back, 0]), int(rng[i, c, back, 1])
                row = off[i, c, back]
                held = {k: int(row[k - kmin]) for k in range(max(lo, kmin), min(hi, kmin + len(row) - 1) + 1) if row[k - kmin] != oracle.ROW_NULL}
                assert all(row[x] == oracle.ROW_NULL for x in range(len(row)) if not lo <= x + kmin <= hi)   # nothing outside the row's range
                assert (c, s - back) not in out or out[(c, s - back)] == held                             # (scores two calls share)
                out[(c, s - back)] = held
    return out


def test_forward_rows_reach_the_end_at_the_dp_score_and_never_step_back(oracle):
    pairs = [(p, t) for p, t in _rand_pairs(23, 260, [1, 2, 7, 40, 64, 100, 101], [0.0, 0.02, 0.1, 0.3]) if p and t]
    assert len(pairs) >= 200
    for p, t in pairs:
        dp = oracle.dp_score(p, t)
        rows = _all_rows(oracle, p, t, dp)
        kinv = len(t) - len(p)
        first = min((s for (c, s), r in rows.items() if c == 0 and r.get(kinv, -1) >= len(t)), default=None)
        assert first == dp, (len(p), len(t), dp, first)
        # Offsets on a diagonal never decrease with the score -- from a score to the one a mismatch later, which is how a row is made of an
        # earlier one: M[s][k] >= M[s - x][k] + 1.  (Not from s - 1 to s: the rows of two consecutive scores
        # have different sources, and M[25][k] out of a gap opened at score 0 can lie beyond M[26][k].)  So the largest of x consecutive rows never
        # decreases, and no row holds less than the gap rows of its score.
        x = oracle.DEFAULT_PEN[0]
        for s in range(x, dp + 1):
            before, now = rows[(0, s - x)], rows[(0, s)]
            for k, v in before.items():
                # (where the later row holds the diagonal at all: a cell whose largest source lies beyond the rectangle is nulled as a whole)
                assert k not in now or now[k] >= v + 1, (s, k)
        for s in range(dp + 1):
            for c in range(1, 5):
                assert all(rows[(0, s)].get(k, v) >= v for k, v in rows[(c, s)].items()), (c, s)
        for (c, s), r in rows.items():   # every offset inside the rectangle for M; a row never holds a diagonal its score cannot reach
            assert all(abs(k) <= s for k in r)
            if c == 0:
                assert all(0 <= v <= len(t) and 0 <= v - k <= len(p) for k, v in r.items())

