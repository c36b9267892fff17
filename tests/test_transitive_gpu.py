"""GPU tests of the transitive closure: wfm_trans_* through capi.Transitive, every interval and every per-seed row held against the brute
force of tests/trans_model.py, at the smallest shapes at which each part can go wrong."""
import random

import numpy as np
import pytest

from tests import lift_model as LM
from tests import trans_model as TM
from tests.test_transitive_cpu import random_world
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

SPANS = capi.WFM_TRANS_SPANS


def rec(t, q, cigar, rev=False):
    return (t, q, rev, LM.parse(cigar) if isinstance(cigar, str) else cigar)


def _add(obj, records, n_bases):
    probs, words = TM.problems(records)
    flags = obj.add(probs, words)
    assert flags.tolist() == [0 if TM.good(r, n_bases) else SPANS for r in records]


def _closure(obj, seeds, depth):
    ivs, per = obj.closure(seeds, depth)
    assert ivs.dtype.itemsize == 24 and not ivs["pad_"].any()
    return (list(zip(ivs["start"].tolist(), ivs["end"].tolist(), ivs["seed"].tolist())),
            list(zip(per["first"].tolist(), per["count"].tolist(), per["bases"].tolist())), ivs.tobytes())


def _check(obj, records, n_bases, seeds, depth):
    """the closure of an object that holds `records`, held against the model; returns the result's bytes"""
    kept = [r for r in records if TM.good(r, n_bases)]
    want_ivs, want_per, want_rounds = TM.closures(kept, seeds, depth)
    got_ivs, got_per, raw = _closure(obj, seeds, depth)
    assert got_ivs == want_ivs
    assert got_per == want_per
    c = obj.counts()
    assert c[0] == len(kept) and c[2] == 2 * len(kept) and c[1] == sum(len(r[3]) + 1 for r in kept)
    assert c[3] == want_rounds and c[4] == len(want_ivs)
    return raw


def _fresh(gpu, records, n_bases, seeds, depth, calls=1):
    obj = gpu.transitive(n_bases)
    try:
        step = max(1, (len(records) + calls - 1) // calls)
        for a in range(0, len(records), step):
            _add(obj, records[a:a + step], n_bases)
        return _check(obj, records, n_bases, seeds, depth)
    finally:
        obj.close()


def _subintervals(a, b):
    return [(i, j) for i in range(a, b) for j in range(i + 1, b + 1)]


# ---- the hull ----

@pytest.mark.parametrize("rev", [False, True], ids=["plus", "reverse"])
def test_every_subinterval_of_both_spans(gpu, rev):
    r = rec(5, 40, "3=2I4=1X2D3=", rev)
    P, T = TM.spans(r[3])
    assert (P, T) == (13, 13)
    seeds = _subintervals(5, 5 + P) + _subintervals(40, 40 + T)
    _fresh(gpu, [r], 64, seeds, 1)


@pytest.mark.parametrize("rev", [False, True], ids=["plus", "reverse"])
def test_600_runs_cross_the_rounds_of_256(gpu, rev):
    runs = LM.parse("1=1I1=1D" * 150)
    assert len(runs) == 600
    P, T = TM.spans(runs)
    r = rec(10, 1000, runs, rev)
    pre_p, pre_t, p, t = [], [], 0, 0
    for n, op in runs:
        pre_p.append(p)
        pre_t.append(t)
        p += n if op != "I" else 0
        t += n if op != "D" else 0
    seeds = []
    for k in (254, 255, 256, 257, 258, 511, 512, 513, 598, 599):
        seeds += [(10 + pre_p[k], 10 + pre_p[k] + 1), (10 + max(0, pre_p[k] - 1), 10 + min(P, pre_p[k] + 2))]
        ti = pre_t[k]
        for a, b in ((ti, ti + 1), (max(0, ti - 1), min(T, ti + 2))):
            seeds.append((1000 + T - b, 1000 + T - a) if rev else (1000 + a, 1000 + b))
    seeds += [(10, 10 + P), (1000, 1000 + T), (10 + pre_p[200], 10 + pre_p[300]), (1000 + 150, 1000 + 300)]
    _fresh(gpu, [r], 2000, seeds, 1)


def test_an_interval_inside_a_gap_run_gives_nothing(gpu):
    r = rec(10, 100, "3=4D3=4I3=")
    # target bases 13 .. 16 are the D run; text indices 6 .. 9 the I run
    seeds = [(14, 16), (13, 17), (106, 110), (107, 109)]
    raw = _fresh(gpu, [r], 200, seeds, 1)
    ivs = np.frombuffer(raw, dtype=capi.TRANS_IV_DTYPE)
    assert list(zip(ivs["start"].tolist(), ivs["end"].tolist())) == seeds
    rr = rec(10, 100, "3=4D3=4I3=", True)
    _fresh(gpu, [rr], 200, seeds + [(100, 104), (103, 107)], 1)


@pytest.mark.parametrize("cigar", ["5=", "1X", "2I", "3D"])
def test_tiny_records(gpu, cigar):
    r = rec(3, 20, cigar)
    _fresh(gpu, [r, rec(3, 20, cigar, True)], 32, _subintervals(0, 10) + _subintervals(18, 27), 2)


# ---- the arc window ----

def test_one_long_arc_over_300_short_ones(gpu):
    records = [rec(0, 10000, "2000=")] + [rec(100 + 5 * i, 20000 + 10 * i, "3=") for i in range(300)]
    last = 100 + 5 * 299
    seeds = [(50, 60), (1700, 1710), (last, last + 3), (last + 1, last + 2), (99, 101), (0, 2000), (20000, 23000)]
    _fresh(gpu, records, 30000, seeds, 1)
    _fresh(gpu, records, 30000, seeds[:4], 2)


def test_arcs_that_abut_the_seed_are_not_taken(gpu):
    a, b = 50, 60
    records = [rec(a - 3, 100, "3="), rec(b, 200, "3="), rec(300, a - 4, "4="), rec(400, b, "4=")]
    raw = _fresh(gpu, records, 500, [(a, b), (a - 1, b), (a, b + 1)], 1)
    ivs = np.frombuffer(raw, dtype=capi.TRANS_IV_DTYPE)
    assert [(int(v["start"]), int(v["end"])) for v in ivs if v["seed"] == 0] == [(a, b)]


# ---- the closure ----

CHAIN = [rec(10, 1010, "20=2I20=3D20="), rec(1000, 2005, "30=1X40=", True), rec(2000, 3020, "25=4D25=2I30=")]


@pytest.mark.parametrize("depth", [1, 2, 3, 0])
def test_a_chain_of_records(gpu, depth):
    seeds = [(20, 30), (3050, 3060), (1030, 1031)]
    raw = _fresh(gpu, CHAIN, 4000, seeds, depth)
    ivs = np.frombuffer(raw, dtype=capi.TRANS_IV_DTYPE)
    reached = {(int(v["seed"]), int(v["start"]) // 1000) for v in ivs}
    # A reaches one more sequence per round; D reaches A through back arcs alone
    assert {r for s, r in reached if s == 0} == set(range(4 if depth == 0 else depth + 1))
    assert ((1, 0) in reached) == (depth in (3, 0))


def test_a_cycle_grows_round_by_round_and_ends(gpu):
    records = [rec(0, 1003, "25=3I25="), rec(1000, 0, "30=3I30=")]
    want, _, rounds = TM.closures(records, [(10, 12)], 0)
    assert rounds > 3
    obj = gpu.transitive(2000)
    try:
        _add(obj, records, 2000)
        _check(obj, records, 2000, [(10, 12)], 0)
        assert obj.counts()[3] == rounds
        for depth in (1, 2, 3, rounds - 1, rounds, rounds + 5):
            _check(obj, records, 2000, [(10, 12), (1040, 1041)], depth)
    finally:
        obj.close()


def test_identical_seeds_stay_two_results(gpu):
    raw = _fresh(gpu, CHAIN, 4000, [(20, 30), (20, 30), (15, 35)], 2)
    ivs = np.frombuffer(raw, dtype=capi.TRANS_IV_DTYPE)
    a = [(int(v["start"]), int(v["end"])) for v in ivs if v["seed"] == 0]
    b = [(int(v["start"]), int(v["end"])) for v in ivs if v["seed"] == 1]
    assert a == b and len(a) >= 3


def test_abutting_hulls_merge_and_hulls_one_base_apart_do_not(gpu):
    raw = _fresh(gpu, [rec(0, 100, "5="), rec(10, 105, "5=")], 300, [(0, 15)], 1)
    ivs = np.frombuffer(raw, dtype=capi.TRANS_IV_DTYPE)
    assert [(int(v["start"]), int(v["end"])) for v in ivs] == [(0, 15), (100, 110)]
    raw = _fresh(gpu, [rec(0, 100, "5="), rec(10, 106, "5=")], 300, [(0, 15)], 1)
    ivs = np.frombuffer(raw, dtype=capi.TRANS_IV_DTYPE)
    assert [(int(v["start"]), int(v["end"])) for v in ivs] == [(0, 15), (100, 105), (106, 111)]


def test_a_seed_no_arc_touches_is_returned_alone(gpu):
    raw = _fresh(gpu, CHAIN, 4000, [(500, 600), (20, 30), (3990, 4000)], 0)
    ivs = np.frombuffer(raw, dtype=capi.TRANS_IV_DTYPE)
    assert [(int(v["start"]), int(v["end"])) for v in ivs if v["seed"] != 1] == [(500, 600), (3990, 4000)]
    obj = gpu.transitive(100)
    try:
        assert _closure(obj, [(1, 5), (0, 100)], 0)[0] == [(1, 5, 0), (0, 100, 1)]
        assert obj.counts()[3] == 0
        assert _closure(obj, [], 2)[0] == []
    finally:
        obj.close()


def test_random_worlds(gpu):
    rng = random.Random(0x7e)
    for _ in range(12):
        records = random_world(rng, 200, 6)
        seeds = []
        for _ in range(6):
            a = rng.randint(0, 190)
            seeds.append((a, rng.randint(a + 1, min(200, a + 15))))
        for depth in (0, 1, 2, 3):
            _fresh(gpu, records, 200, seeds, depth)


# ---- the object ----

def _pile(rng, n=40, n_bases=3000):
    """records that pile over the same few hundred bases of four sequences"""
    out = []
    for _ in range(n):
        runs = []
        for k in range(rng.randint(1, 6)):
            runs += [(rng.randint(3, 30), rng.choice("=X")), (rng.randint(1, 5), rng.choice("ID"))]
        runs.append((rng.randint(3, 30), "="))
        P, T = TM.spans(runs)
        out.append((rng.randint(0, 3) * 700 + rng.randint(0, 700 - P), rng.randint(0, 3) * 700 + rng.randint(0, 700 - T), rng.random() < 0.5, runs))
    return out


def test_calls_order_and_merged_objects_give_the_same_bytes(gpu):
    rng = random.Random(0x7f)
    records = _pile(rng)
    seeds = [(100, 140), (800, 820), (2100, 2101), (0, 700)]
    one = _fresh(gpu, records, 3000, seeds, 2)
    assert _fresh(gpu, records, 3000, seeds, 2, calls=3) == one
    shuffled = records[:]
    rng.shuffle(shuffled)
    assert _fresh(gpu, shuffled, 3000, seeds, 2, calls=2) == one
    a, b, c = gpu.transitive(3000), gpu.transitive(3000), gpu.transitive(3000)
    try:
        _add(a, records[:15], 3000)
        _add(b, records[15:30], 3000)
        _add(c, records[30:], 3000)
        for src, part in ((a, records[:15]), (b, records[15:30])):
            recs, words = src.export()
            assert len(recs) == 15 and len(words) == sum(len(r[3]) + 1 for r in part)
            c.import_(recs, words)
        assert _check(c, records, 3000, seeds, 2) == one
        assert _check(c, records, 3000, seeds, 0) == _fresh(gpu, records, 3000, seeds, 0)
        # a second closure after one more add
        more = rec(150, 2900, "20=1I30=")
        _add(c, [more], 3000)
        _check(c, records + [more], 3000, seeds, 2)
        # import looks at everything first: a word list whose prefixes fall is refused and nothing is added
        recs, words = a.export()
        bad = words.copy()
        bad["p"][3] = 0
        with pytest.raises(capi.WfmError, match="nothing was added"):
            c.import_(recs, bad)
        _check(c, records + [more], 3000, seeds, 2)
    finally:
        a.close(); b.close(); c.close()


def test_small_output_chunks_give_the_same_bytes(gpu, monkeypatch):
    rng = random.Random(0x80)
    records = _pile(rng)
    seeds = [(100, 140), (800, 820), (0, 700), (1400, 2100)]
    want = _fresh(gpu, records, 3000, seeds, 3)
    monkeypatch.setenv("WFM_TRANS_OUT_MB", "0.0001")  # six pairs a chunk
    assert _fresh(gpu, records, 3000, seeds, 3) == want
    assert _fresh(gpu, records, 3000, seeds, 0) == _fresh(gpu, records, 3000, seeds, 50)


def test_coordinates_above_2_to_the_33(gpu):
    n_bases = 1 << 34
    hi = (1 << 33) + 12345
    records = [rec(hi, 100, "30=2I30="), rec(hi + 1000, hi + 40, "20=3D20=", True), rec(n_bases - 50, 7, "50=")]
    seeds = [(hi + 5, hi + 15), (110, 120), (n_bases - 10, n_bases), (0, 60)]
    for depth in (1, 2, 0):
        _fresh(gpu, records, n_bases, seeds, depth)


def test_a_refused_problem_between_two_good_ones(gpu):
    n_bases = 1000
    good = [rec(10, 500, "20=2I20="), rec(500, 40, "10=1X10=", True)]
    for bad in (rec(990, 0, "20="), rec(0, 990, "20="), rec(0, 0, [(3, "="), (0, "I"), (3, "=")]), rec(5, 5, []), rec(1001, 0, "1=")):
        records = [good[0], bad, good[1]]
        assert not TM.good(bad, n_bases)
        assert _fresh(gpu, records, n_bases, [(15, 25), (505, 506)], 0) == _fresh(gpu, good, n_bases, [(15, 25), (505, 506)], 0)


def test_argument_errors_leave_the_handle_usable(gpu):
    with pytest.raises(capi.WfmError, match="2\\^40"):
        gpu.transitive(1 << 40)
    obj = gpu.transitive(1000)
    try:
        with pytest.raises(capi.WfmError, match="leave the run buffer"):
            obj.add([(0, 0, 2, 5, 0)], LM.words(LM.parse("3=1I3=")))
        with pytest.raises(capi.WfmError, match="WFM_TRANS_REVERSE"):
            obj.add([(0, 0, 0, 3, 4)], LM.words(LM.parse("3=1I3=")))
        with pytest.raises(capi.WfmError, match="seed 1"):
            obj.closure([(0, 5), (5, 5)], 1)
        with pytest.raises(capi.WfmError, match="seed 0"):
            obj.closure([(990, 1001)], 1)
        assert obj.counts()[0] == 0
        records = [rec(10, 500, "20=2I20=")]
        _add(obj, records, 1000)
        _check(obj, records, 1000, [(15, 25)], 2)
    finally:
        obj.close()


def test_the_cap_names_the_pass(gpu, monkeypatch):
    obj = gpu.transitive(1000)
    try:
        monkeypatch.setenv("WFM_TRANS_GB", "0.0000001")
        with pytest.raises(capi.WfmError, match="transitive.*WFM_TRANS_GB"):
            _add(obj, [rec(10, 500, "20=2I20=")], 1000)
        monkeypatch.delenv("WFM_TRANS_GB")
        assert obj.counts()[:3] == (0, 0, 0)
        _add(obj, [rec(10, 500, "20=2I20=")], 1000)
        _check(obj, [rec(10, 500, "20=2I20=")], 1000, [(15, 25)], 1)
    finally:
        obj.close()


def test_interleaved_with_other_passes_on_one_handle(gpu):
    rng = random.Random(0x81)
    records = _pile(rng, 20)
    seeds = [(100, 140), (800, 820)]
    want = _fresh(gpu, records, 3000, seeds, 2)
    probs, words = TM.problems(records)
    cov = [(t, off, n) for t, q, off, n, fl in probs]
    ls = gpu.liftset([(100, 140), (800, 820)], 3000)
    net = gpu.net(3000)
    obj = gpu.transitive(3000)
    try:
        lifts_alone = ls.lift(cov, words)
        net.add([(t, off, n, capi.WFM_NET_SCORE_EQ, i) for i, (t, off, n) in enumerate(cov)], words)
        table_alone = net.table()
        _add(obj, records[:10], 3000)
        lifts = ls.lift(cov, words)
        _add(obj, records[10:], 3000)
        table = net.table()
        assert _check(obj, records, 3000, seeds, 2) == want
        lifts2 = ls.lift(cov, words)
        table2 = net.table()
        for got in (lifts, lifts2):
            assert got[0].tobytes() == lifts_alone[0].tobytes()
        for got in (table, table2):
            assert got[0].tobytes() == table_alone[0].tobytes() and got[1].tobytes() == table_alone[1].tobytes()
        assert _check(obj, records, 3000, seeds, 2) == want
    finally:
        obj.close(); net.close(); ls.close()
