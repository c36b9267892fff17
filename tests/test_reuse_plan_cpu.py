"""The planning of parent reuse without a GPU (wfmash_amd/csrc/wfa_plan.h through wfmh_test_reuse_plan and wfmh_test_tile_plan_dirs): which of
its parent's keeps a child resumes from, which nodes are refused, the tiles a job gets while one of its directions waits for its keep, and the
cadence of the keeps under the store's cap.  The expected values are worked out here, in Python, from the definitions."""
import ctypes as C
import random

import numpy as np
import pytest

from wfmash_amd import capi

NONE = 1 << 29   # SUB_NONE
BACK = 25        # RNG_BACK
KEEP_ROWS = 32   # 26 rows of M, two of I1 and of D1, one of I2 and of D2
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def L():
    lib = capi.load()
    for name in ("wfmh_test_reuse_plan", "wfmh_test_tile_plan_dirs"):
        assert name in capi.HOST_EXPORTS
        getattr(lib, name).restype = C.c_int
    lib.wfmh_test_reuse_plan.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    lib.wfmh_test_tile_plan_dirs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return lib


def call(L, op, args, n):
    a = np.array(args, dtype=np.int64)
    out = np.zeros(2, dtype=np.int64)
    assert L.wfmh_test_reuse_plan(op, a.ctypes.data, n, out.ctypes.data) == 0
    return int(out[0]), int(out[1])


def pick(L, score_rem, T, margin, kept, min_blocks=1):
    return call(L, 0, [score_rem, T, margin, min_blocks] + list(kept), len(kept))


def eligible(L, child=(3000, 3100), score_rem=900, child_sub=NONE, keep=1, fits=1, tile_it=1, band=0, grown=0, parent=(8000, 8200, NONE), s_k=200, T=100):
    return call(L, 1, [child[0], child[1], score_rem, child_sub, keep, fits, tile_it, band, grown, parent[0], parent[1], parent[2], s_k, T], 0)[0]


# ---- the keep a child resumes from ----

def test_the_keep_picked_is_the_newest_within_the_two_inequalities(L):
    rnd = random.Random(7)
    for _ in range(400):
        T = rnd.choice([32, 64, 100])
        margin = rnd.choice([0, 48, 100])
        score = rnd.randrange(0, 9000)
        cad = rnd.choice([1, 2, 4]) * T
        kept = list(range(cad, rnd.randrange(cad, 6000) + 1, cad))
        rnd.shuffle(kept)
        idx, limit = pick(L, score, T, margin, kept)
        x = score // 2 - margin
        want_limit = -1 if x < 0 else x // T * T - T   # floor_T(score / 2 - fine_margin) - T
        assert limit == want_limit
        ok = [s for s in kept if T <= s <= want_limit]
        if not ok:
            assert idx == -1
        else:
            assert kept[idx] == max(ok)
            # the meeting block (the one that holds score / 2 - margin .. ) is never the first after the restore
            assert kept[idx] + T <= x


def test_a_child_of_c3_depth_resumes_where_the_issue_says(L):
    # a child of score 3400 under T = 100, margin 48, keeps every two blocks: floor_100(1700 - 48) - 100 = 1500 -> the keep of 1400
    kept = list(range(200, 3401, 200))
    idx, limit = pick(L, 3400, 100, 48, kept)
    assert limit == 1500 and kept[idx] == 1400
    # keeps of every block: the one of 1500 itself
    kept = list(range(100, 3401, 100))
    assert kept[pick(L, 3400, 100, 48, kept)[0]] == 1500


def test_no_keep_for_a_node_without_a_score_or_a_shallow_one(L):
    kept = list(range(200, 2001, 200))
    assert pick(L, INT_MAX, 100, 48, kept) == (-1, -1)
    assert pick(L, 500, 100, 48, kept)[0] == -1          # floor_100(250 - 48) - 100 = 100 < 200
    assert pick(L, 700, 100, 48, kept)[0] == 0           # floor_100(350 - 48) - 100 = 200
    assert pick(L, 3000, 100, 48, [])[0] == -1
    # WFM_REUSE_MIN_BLOCKS: a keep fewer blocks deep than that is not taken -- floor_100(1100 - 48) - 100 = 900: the keep of 800 is, under 9 blocks none
    assert pick(L, 2200, 100, 48, kept, min_blocks=8)[0] == kept.index(800) and pick(L, 2200, 100, 48, kept, min_blocks=9)[0] == -1


# ---- the nodes that are refused ----

def test_nodes_that_may_not_resume(L):
    assert eligible(L) == 1
    assert eligible(L, keep=0) == 0                       # came without a keep
    assert eligible(L, score_rem=INT_MAX) == 0            # does not know its score
    assert eligible(L, band=700) == 0                     # on a narrow ring
    assert eligible(L, band=700, grown=1) == 0 and eligible(L, grown=1) == 0
    assert eligible(L, tile_it=0) == 0 and eligible(L, fits=0) == 0
    assert eligible(L, s_k=0) == 0 and eligible(L, s_k=50) == 0 and eligible(L, s_k=250) == 0   # no block boundary from T on


def test_the_parents_rows_must_hold_the_childs(L):
    # the parent's rows were cut by a bound of its score; the child (no bound of its own binds) would need diagonals beyond them
    # parent 8000 x 8200, sub 300: rows hold |k - 200| <= 300 - s; at s = 200 that is [100, 200] clipped to [-200, 200]
    assert eligible(L, parent=(8000, 8200, 300), s_k=200) == 0
    # a bound far away cuts nothing at these scores
    assert eligible(L, parent=(8000, 8200, 5000), s_k=200) == 1
    # the child's own bound cuts its rows to inside the parent's: kinv_c = 100, sub_c = 320 -> at s = 200 [-20, 200] ... the parent [-200, 200]
    assert eligible(L, child=(3000, 3100), child_sub=320, parent=(8000, 8200, NONE), s_k=200) == 1
    # brute force over random boxes: containment at every score the keep's rows span
    rnd = random.Random(11)
    for _ in range(300):
        ppl, ptl = rnd.randrange(400, 3000), rnd.randrange(400, 3000)
        cpl, ctl = rnd.randrange(100, ppl + 1), rnd.randrange(100, ptl + 1)
        psub = rnd.choice([NONE, rnd.randrange(100, 2500)])
        csub = rnd.choice([NONE, rnd.randrange(100, 2500)])
        s_k = rnd.randrange(1, 12) * 100

        def rng(pl, tl, sub, s):
            return max(-pl, -s, (tl - pl) - sub + s), min(tl, s, (tl - pl) + sub - s)
        want = 1
        for s in range(max(0, s_k - BACK), s_k + 1):
            clo, chi = rng(cpl, ctl, csub, s)
            plo, phi = rng(ppl, ptl, psub, s)
            if chi >= clo and (clo < plo or chi > phi):
                want = 0
        assert eligible(L, child=(cpl, ctl), child_sub=csub, parent=(ppl, ptl, psub), s_k=s_k) == want, (ppl, ptl, psub, cpl, ctl, csub, s_k)


# ---- the tiles of a job one of whose directions waits ----

def tile_plan_dirs(L, jobs, dirs, threads=512, Cc=2, T=100, chunk=2):
    core = threads * Cc - 2 * T
    j = np.array(jobs, dtype=np.int32).reshape(-1, 8)
    d = np.array(dirs, dtype=np.uint8)
    rules = np.array([threads, Cc, T, chunk, core, 1, 1, 0], dtype=np.int32)
    per_block = np.zeros(2 * chunk, dtype=np.int32)
    cap = 1 << 14
    tasks = np.zeros((cap, 4), dtype=np.int32)
    sc = np.zeros(3, dtype=np.int64)
    assert L.wfmh_test_tile_plan_dirs(j.ctypes.data, len(j), rules.ctypes.data, d.ctypes.data, per_block.ctypes.data, tasks.ctypes.data, cap, sc.ctypes.data) == 0
    return [tuple(t) for t in tasks[:sc[1]].tolist()], int(sc[2])


def test_only_the_inner_direction_has_tiles_below_the_keep_and_both_from_it_on(L):
    # (pl, tl, sub, s0, mode, fine_s, packed, active); job 1 waits for a forward keep at 1400 (its reverse direction runs alone), job 2 for a reverse one
    s_k = 1400
    for s0 in (0, 600, 1200, 1400, 1600):
        jobs = [(25000, 25100, NONE, s0, 0, INT_MAX, 1, 1), (24000, 24100, NONE, s0, 0, INT_MAX, 1, 1), (9000, 9050, NONE, s0, 0, INT_MAX, 0, 1)]
        dirs = [3, 2 if s0 < s_k else 3, 1 if s0 < s_k else 3]
        tasks, n_pk = tile_plan_dirs(L, jobs, dirs)
        both, _ = tile_plan_dirs(L, jobs, [3, 3, 3])
        for job in range(3):
            mine = [t for t in tasks if t[0] == job]
            full = [t for t in both if t[0] == job]
            want = [t for t in full if (dirs[job] >> t[1]) & 1]
            assert mine == want and len(want) > 0
            if dirs[job] != 3:
                assert {t[1] for t in mine} == {1 if dirs[job] == 2 else 0} and 2 * len(mine) == len(full)
        assert n_pk == sum(1 for t in tasks if t[0] != 2)       # the byte kernel's tiles stay behind the packed ones
        assert all(t[0] != 2 for t in tasks[:n_pk]) and all(t[0] == 2 for t in tasks[n_pk:])


# ---- the cadence ----

def cadence(L, every, chunk, T, cap, keepers):
    flat = [every, chunk, T, cap]
    for k in keepers:
        flat += list(k)
    return call(L, 2, flat, len(keepers))


def keep_bytes(pl, tl, upto, cad, T):
    """both directions of every keep up to `upto`: KEEP_ROWS rows over the diagonals [max(-pl, -s), min(tl, s)]"""
    return sum(2 * 4 * KEEP_ROWS * (min(tl, s) - max(-pl, -s) + 1) for s in range(cad * T, upto + 1, cad * T))


def test_the_cadence_is_whole_chunks_and_doubles_under_a_small_budget(L):
    assert cadence(L, 1, 2, 100, 1 << 40, [(50000, 50000, 3000)]) == (2, 2)     # a keep is taken where the host looks
    assert cadence(L, 2, 2, 100, 1 << 40, [(50000, 50000, 3000)]) == (2, 2)
    assert cadence(L, 4, 2, 100, 1 << 40, [(50000, 50000, 3000)]) == (4, 4)
    assert cadence(L, 3, 2, 100, 1 << 40, [(50000, 50000, 3000)]) == (4, 4)
    assert cadence(L, 1, 1, 32, 1 << 40, [(5000, 5000, 800)]) == (1, 1)
    keepers = [(50000, 50000, 3000)] * 21
    full = sum(keep_bytes(*k, 2, 100) for k in keepers)
    assert cadence(L, 2, 2, 100, full, keepers) == (2, 2)
    got = cadence(L, 2, 2, 100, full - 1, keepers)[1]
    assert got == 4 and sum(keep_bytes(*k, 4, 100) for k in keepers) <= full - 1
    # the smallest cadence that fits, by doubling
    for cap in (full // 3, full // 7, full // 20):
        got = cadence(L, 2, 2, 100, cap, keepers)[1]
        want = 2
        while want * 100 <= 3000 and sum(keep_bytes(*k, want, 100) for k in keepers) > cap:
            want *= 2
        assert got == (want if want * 100 <= 3000 else 0)
    # below one keep a job: no reuse in the chunk
    assert cadence(L, 2, 2, 100, 1000, keepers)[1] == 0
    assert cadence(L, 2, 2, 100, 1 << 40, [(50000, 50000, 100)])[1] == 0


# ---- the keeps worth their copy ----

def test_keeps_are_written_around_half_the_meeting_score_only(L):
    """a job of A = 100 k antidiagonals whose directions gain 6.5 antidiagonals a score each: they meet at 7692; its children resume near 3800"""
    A, T, cad = 100000, 100, 2
    s_meet = 7692
    wanted = [es for es in range(200, 7601, 200) if call(L, 3, [es - 200, es, 13 * (es - 200), A, cad, T], 0)[0]]
    lo, hi = 0.4 * s_meet - 64 - (2 + cad) * T, 0.6 * s_meet
    assert wanted == [es for es in range(200, 7601, 200) if es - 200 > 0 and lo - 1 <= es <= hi + 1]
    # every score a child of half the job's score can resume at, whatever the rounding: floor_T(c / 2 - 48) - T and a cadence below it
    for c in range(s_meet - 30, s_meet + 30):
        limit = pick(L, c, T, 48, [])[1]
        newest = limit // (cad * T) * (cad * T)
        assert newest in wanted, (c, limit, newest)
    # nothing before the job has moved, nothing without progress
    assert call(L, 3, [0, 200, 0, A, cad, T], 0)[0] == 0 and call(L, 3, [200, 400, 0, A, cad, T], 0)[0] == 0
