"""The arithmetic of the BiWFA level driver without a GPU (wfmash_amd/csrc/wfa_plan.h through wfmh_test_ring_plan and
wfmh_test_expand_runs): which ring a job gets under a memory budget -- full, guessed band, grown band, on the tile kernels or
on the step kernel alone, or none (WFM_ST_OOM) -- and how a problem's runs become its op string.

The expected values of the hand-derived cases were worked out on paper from the rules, not read off
the code under test.  One column of a ring of 32 rows is 2 directions x 5 components x 32 rows x 4 B = 1280 B."""
import random

from wfmash_amd import capi
from wfmash_amd.capi import SCORE_NONE, SUB_NONE, expand_runs, ring_plan

MiB = 1 << 20
OP_M, OP_X, OP_I, OP_D = 0, 1, 2, 3


def _full(pl, tl):
    return (pl + tl + 9 + 3) & ~3


# ---- hand-derived cases ----

def test_root_on_its_guessed_band():
    """80 kbp a side, nothing known, the level over a budget of 128 MiB: band 4096 + 2 x 100 + 16 = 4312, the ring holds
    |k| <= 4320: 80000 - 4320 = 75680 columns cut on the left, 4320 + 4320 + 9 -> 8652 columns, k = 0 in column 4324."""
    p = ring_plan(80_000, 80_000, 128 * MiB, use_band=True, over_budget=True)
    assert p == dict(width=8652, koff=4324, band=4312, tile_it=True, grown=False, need=8652 * 320 * 2)


def test_root_after_its_band_failed_grows_fourfold():
    """The full ring is 160 012 columns = 204.8 MB: it does not fit, the band grows to 4 x 4312 = 17 248.  80000 - 17256 = 62744
    cut, 17256 + 17256 + 9 -> 34 524 columns, k = 0 in column 17 260; two such rings are 88.4 MB: tile kernels."""
    assert _full(80_000, 80_000) == 160_012 and 160_012 * 1280 > 128 * MiB
    p = ring_plan(80_000, 80_000, 128 * MiB, noband=1, band=4312, use_band=True, over_budget=True)
    assert p == dict(width=34_524, koff=17_260, band=17_248, tile_it=True, grown=True, need=34_524 * 320 * 2)
    assert 2 * 34_524 * 1280 <= 128 * MiB


def test_root_under_one_mib_is_clamped_to_what_the_budget_holds():
    """The guessed band's ring (8652 columns, 11 MB) does not fit, nor does one for 4096 scores (8220 columns): the band is what
    819 columns allow, (819 - 32) / 2 = 393: 80000 - 401 -> 79596 cut, 404 + 401 + 9 -> 816 columns, k = 0 in column 408."""
    p = ring_plan(80_000, 80_000, 1 * MiB, use_band=True, over_budget=True)
    assert p == dict(width=816, koff=408, band=393, tile_it=False, grown=True, need=816 * 320)
    assert ring_plan(80_000, 80_000, 1 * MiB, noband=1, band=393, use_band=True, over_budget=True) is None  # the clamp cannot pass the band it had


def test_child_of_known_score():
    """score 1000: 500 + 64 scores a direction + 216 = 780; the ring holds |k| <= 788."""
    # 5000 x 5000: 5000 - 788 = 4212 cut, 788 + 788 + 9 -> 1588 columns (a sixth of the 10 012), k = 0 in column 792
    p = ring_plan(5000, 5000, 1024 * MiB, score_rem=1000, sub=1032, use_band=True)
    assert p == dict(width=1588, koff=792, band=780, tile_it=True, grown=False, need=1588 * 320 * 2)
    # 700 x 9000: the pattern is shorter than the band's reach, nothing to cut on the left: the guess is refused, the ring stays full
    p = ring_plan(700, 9000, 1024 * MiB, score_rem=1000, sub=1032, use_band=True)
    assert p == dict(width=9712, koff=704, band=0, tile_it=True, grown=False, need=9712 * 320 * 2)


def test_short_or_cheap_jobs_are_never_tiled():
    p = ring_plan(60, 60, 1024 * MiB, use_band=True, over_budget=True)  # 120 < min_len 128
    assert p == dict(width=132, koff=64, band=0, tile_it=False, grown=False, need=132 * 320)
    p = ring_plan(5000, 5000, 1024 * MiB, score_rem=50, sub=82, use_band=True)  # 50 < min_score 64
    assert p == dict(width=10_012, koff=5004, band=0, tile_it=False, grown=False, need=10_012 * 320)
    p = ring_plan(5000, 5000, 1024 * MiB, score_rem=1000, tiles=False, use_band=True)
    assert p == dict(width=10_012, koff=5004, band=0, tile_it=False, grown=False, need=10_012 * 320)


def test_deep_rings_same_geometry_four_times_the_bytes():
    """128 rows: a column is 5120 B.  Under 64 MiB the two rings of the guessed band fit at 32 rows (22 MB) and not at 128
    (88.6 MB), where the one ring of the step kernel does (44.3 MB)."""
    a = ring_plan(80_000, 80_000, 64 * MiB, use_band=True, over_budget=True)
    b = ring_plan(80_000, 80_000, 64 * MiB, use_band=True, over_budget=True, RR=128)
    assert a == dict(width=8652, koff=4324, band=4312, tile_it=True, grown=False, need=8652 * 320 * 2)
    assert b == dict(width=8652, koff=4324, band=4312, tile_it=False, grown=False, need=8652 * 1280)


# ---- band_geometry against a formula of its own ----

def _geometry(pl, tl, b):
    """A ring for |k| <= b + 8 with 4 columns to the left of its first diagonal: (columns cut on the left, columns, column of k = 0).
    Written from the rule, in other terms than the header: the first diagonal kept is the cut minus pl."""
    reach = b + 8
    cut = max(0, (pl - reach) // 4 * 4)
    k_first, k_last = cut - pl, min(tl, reach)
    cols = k_last - k_first + 1 + 4 + 4  # the diagonals, the left margin, 4 to spare on the right
    return cut, (cols + 3) // 4 * 4, 4 - k_first


def _guessed(pl, tl, b, budget=1 << 40):
    """A root whose guessed band is exactly b (WFM_BAND_ROOT = b - 16, no chunk of blocks on top)."""
    return ring_plan(pl, tl, budget, use_band=True, over_budget=True, band_root=b - 16, chunk=0, T=0, min_len=0)


def _grown(pl, tl, b, budget):
    """A root that had no band and whose full ring does not fit: its first grown band is WFM_BAND_ROOT = b."""
    return ring_plan(pl, tl, budget, noband=1, band_root=b)


def test_band_geometry_and_its_two_acceptance_rules_at_their_edges():
    rng = random.Random(11)
    n = 0
    for _ in range(2000):
        pl, tl, b = rng.randrange(1, 60_000), rng.randrange(1, 60_000), rng.randrange(64, 30_000)
        cut, w, koff = _geometry(pl, tl, b)
        full = _full(pl, tl)
        p = _guessed(pl, tl, b)
        if cut > 0 and 2 * w <= full:
            assert (p["band"], p["width"], p["koff"], p["grown"]) == (b, w, koff, False), (pl, tl, b, p)
        else:
            assert (p["band"], p["width"], p["koff"]) == (0, full, pl + 4), (pl, tl, b, p)
        budget = full * 1280 - 1  # the full ring just does not fit
        p = _grown(pl, tl, b, budget)
        if w < full:
            assert p is not None and (p["band"], p["width"], p["koff"], p["grown"]) == (b, w, koff, True), (pl, tl, b, p)
        else:
            assert p is None, (pl, tl, b, p)
        n += 1
    assert n == 2000
    # guessed band, 2 w == full width: b = 1000 -> 2 x 1008 + 9 -> 2028 columns; 2024 x 2020 is a full ring of 4056: taken; one chunk less: refused
    b = 1000
    assert _geometry(2024, 2020, b)[1] * 2 == 4056 == _full(2024, 2020)
    assert _guessed(2024, 2020, b)["band"] == b and _guessed(2024, 2020, b)["width"] == 2028
    assert _geometry(2024, 2016, b)[1] * 2 == _full(2024, 2016) + 4 and _guessed(2024, 2016, b)["band"] == 0
    # guessed band, shift == 0: pl within 4 of b + 8 -> nothing cut, refused; from b + 12 on a chunk is cut
    assert _geometry(b + 11, 50_000, b)[0] == 0 and _guessed(b + 11, 50_000, b)["band"] == 0
    assert _geometry(b + 12, 50_000, b)[0] == 4 and _guessed(b + 12, 50_000, b)["band"] == b
    # grown band, shift clamped to 0 (short pattern): the ring is cut on the right only
    p = _grown(500, 50_000, b, _full(500, 50_000) * 1280 - 1)
    assert (p["band"], p["width"], p["koff"]) == (b, (500 + b + 8 + 9 + 3) & ~3, 504)
    # grown band, w == full width - 4 is the widest that is taken, w == full width is WFM_ST_OOM
    pl, tl = 500, b + 8 + 4  # diagonals up to b + 8 of tl: one 16-byte chunk less than the full ring
    assert _geometry(pl, tl, b)[1] == _full(pl, tl) - 4
    assert _grown(pl, tl, b, _full(pl, tl) * 1280 - 1)["width"] == _full(pl, tl) - 4
    assert _geometry(pl, tl - 4, b)[1] == _full(pl, tl - 4) and _grown(pl, tl - 4, b, _full(pl, tl - 4) * 1280 - 1) is None


# ---- properties over random nodes ----

def test_properties_over_random_nodes():
    rng = random.Random(7)
    n_checked = n_plans = n_grown = n_oom = n_band = 0
    for _ in range(4000):
        pl, tl = rng.choice([rng.randrange(1, 400), rng.randrange(1, 20_000), rng.randrange(1, 200_000)]), rng.randrange(1, 200_000)
        root = rng.random() < 0.4
        score_rem = SCORE_NONE if root else rng.randrange(0, 40_000)
        sub = SUB_NONE if rng.random() < 0.5 else rng.randrange(1, 60_000)
        noband = int(rng.random() < 0.4)
        band = rng.choice([0, 393, 780, 4312, 17_248, rng.randrange(1, 100_000)]) if noband else 0
        RR = rng.choice([32, 128])
        budget = rng.choice([1, 16, 128, 512, 4096]) * MiB + rng.randrange(0, 4096)
        use_band, over_budget, roots_off = rng.random() < 0.6, rng.random() < 0.5, rng.random() < 0.2
        band_root = rng.choice([4096, 200, 64, 20_000])
        p = ring_plan(pl, tl, budget, score_rem=score_rem, sub=sub, noband=noband, band=band, RR=RR, use_band=use_band,
                      over_budget=over_budget, roots_off=roots_off, band_root=band_root)
        full = _full(pl, tl)
        col = 2 * 5 * RR * 4
        clamp = (budget // col - 32) // 2
        n_checked += 1
        if p is None:  # only where the full ring does not fit either
            n_oom += 1
            assert full * col > budget
            continue
        n_plans += 1
        ctx = (pl, tl, score_rem, sub, noband, band, RR, budget, use_band, over_budget, roots_off, band_root, p)
        assert p["width"] % 4 == 0, ctx
        assert (p["koff"] - (pl + 4)) % 4 == 0, ctx
        assert p["width"] <= full, ctx
        assert p["need"] == p["width"] * 2 * 5 * RR * (2 if p["tile_it"] else 1), ctx
        assert p["need"] * 4 <= budget, ctx
        if p["band"] > 0:
            n_band += 1
            lo, hi = max(-pl, -(p["band"] + 8)), min(tl, p["band"] + 8)
            assert lo + p["koff"] >= 4 and hi + p["koff"] < p["width"], ctx  # every diagonal of the band has its column, 4 to the left
            assert lo + p["koff"] < 8 or lo == -pl, ctx                      # ... and no more than a chunk is wasted there
        else:
            assert (p["width"], p["koff"], p["grown"]) == (full, pl + 4, False), ctx
        if p["grown"]:
            n_grown += 1
            assert p["band"] > band, ctx
            assert p["band"] >= 4 * band or p["band"] == clamp, ctx
        if not use_band and full * col <= budget:
            assert (p["band"], p["width"], p["grown"]) == (0, full, False), ctx
    assert n_checked == 4000 and n_plans + n_oom == 4000
    assert n_grown > 200 and n_oom > 20 and n_band > 500, (n_grown, n_oom, n_band)  # the sweep reaches every regime


# ---- expand_runs ----

def _run(n, op):
    return (n << 2) | op


def _spell(runs):
    return b"".join(b"MXID"[r & 3:(r & 3) + 1] * (r >> 2) for r in runs)


def _score(ops, pen):
    x, o1, e1, o2, e2 = pen
    s, i = 0, 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j] == ops[i]:
            j += 1
        if ops[i:i + 1] == b"X":
            s += x * (j - i)
        elif ops[i:i + 1] in (b"I", b"D"):
            s += min(o1 + e1 * (j - i), o2 + e2 * (j - i))
        i = j
    return s


def _spans(runs):
    pc = sum(r >> 2 for r in runs if r & 3 in (OP_M, OP_X, OP_D))
    tc = sum(r >> 2 for r in runs if r & 3 in (OP_M, OP_X, OP_I))
    return pc, tc


def test_expand_merges_adjacent_runs_in_both_forms():
    runs = [_run(3, OP_M), _run(4, OP_M), _run(1, OP_X), _run(2, OP_I), _run(5, OP_I), _run(2, OP_M), _run(1, OP_D)]
    pc, tc = _spans(runs)
    rc, score, n_runs, ops_len, ops = expand_runs(runs, pc, tc)
    assert (rc, n_runs, ops_len, ops) == (0, 5, 18, b"MMMMMMM" + b"X" + b"IIIIIII" + b"MM" + b"D")
    assert score == 5 + (8 + 2 * 7) + (8 + 2 * 1)
    rc, score_r, n_runs_r, ops_len_r, vec = expand_runs(runs, pc, tc, rle=True, before=(77,))
    assert (rc, score_r, n_runs_r) == (0, score, 5)
    assert vec == [77, _run(7, OP_M), _run(1, OP_X), _run(7, OP_I), _run(2, OP_M), _run(1, OP_D)]
    assert ops_len_r == len(_spell(runs)) == ops_len


def test_expand_scores_with_the_cheaper_gap_piece():
    runs = [_run(10, OP_M), _run(40, OP_D), _run(2, OP_X), _run(3, OP_I), _run(10, OP_M)]
    pc, tc = _spans(runs)
    # default penalties: a gap of 40 costs min(8 + 80, 24 + 40) = 64, one of 3 min(14, 27) = 14
    assert expand_runs(runs, pc, tc)[1] == 64 + 10 + 14
    assert expand_runs(runs, pc, tc, rle=True)[1] == 64 + 10 + 14
    # (3, 10, 3, 2, 1): the second piece is cheaper from the first base on: 2 + 40 and 2 + 3
    assert expand_runs(runs, pc, tc, pen=(3, 10, 3, 2, 1))[1] == 42 + 6 + 5


def test_expand_errors():
    runs = [_run(5, OP_M), _run(2, OP_I), _run(5, OP_M)]
    pc, tc = _spans(runs)
    for plen, tlen in ((pc + 1, tc), (pc, tc - 1)):  # spans do not match: the error, and the run vector as it was
        assert expand_runs(runs, plen, tlen)[0] == 1
        rc, _, _, _, vec = expand_runs(runs, plen, tlen, rle=True, before=(9, 13))
        assert rc == 1 and vec == [9, 13]
    assert expand_runs(runs, pc, tc, ops_cap=11)[0] == 2  # one byte short
    assert expand_runs(runs, pc, tc, ops_cap=12)[0] == 0
    # a run of 2^30 (two entries of 2^29 that merge) has no (len << 2) | op in 32 bits: the run-length form refuses it.  The op form has
    # no such limit -- with an arena of a few bytes it reports the arena, not the run
    big = [_run(1 << 29, OP_M), _run(1 << 29, OP_M)]
    assert expand_runs(big, 1 << 30, 1 << 30, rle=True)[0] == 3
    assert expand_runs(big, 1 << 30, 1 << 30, ops_cap=16)[0] == 2
    ok = [_run(1 << 29, OP_M), _run((1 << 29) - 1, OP_M)]
    rc, score, n_runs, ops_len, vec = expand_runs(ok, (1 << 30) - 1, (1 << 30) - 1, rle=True)
    assert (rc, score, n_runs, ops_len, vec) == (0, 0, 1, (1 << 30) - 1, [_run((1 << 30) - 1, OP_M)])


def test_expand_random_run_lists_both_forms_agree_with_the_spelled_string():
    rng = random.Random(3)
    n = 0
    for trial in range(1500):
        runs = [_run(rng.randrange(1, 40), rng.randrange(0, 4)) for _ in range(rng.randrange(0, 30))]
        pen = capi.DEFAULT_PEN if trial % 3 else (rng.randrange(1, 9), rng.randrange(0, 12), rng.randrange(1, 5), rng.randrange(0, 40), rng.randrange(1, 3))
        pc, tc = _spans(runs)
        want = _spell(runs)
        rc, score, n_runs, ops_len, ops = expand_runs(runs, pc, tc, pen=pen)
        assert (rc, ops, ops_len, score) == (0, want, len(want), _score(want, pen)), (trial, runs)
        rc, score_r, n_runs_r, ops_len_r, vec = expand_runs(runs, pc, tc, pen=pen, rle=True)
        assert (rc, score_r, n_runs_r, ops_len_r) == (0, score, n_runs, len(want)), (trial, runs)
        assert _spell(vec) == want and len(vec) == n_runs and all((a & 3) != (b & 3) for a, b in zip(vec, vec[1:])), (trial, runs)
        n += 1
    assert n == 1500
