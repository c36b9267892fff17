"""The planning of the tile phase, of phase 2 and of the base jobs without a GPU (wfmash_amd/csrc/wfa_rows.h and wfa_plan.h through
wfmh_test_rows, wfmh_test_tile_plan, wfmh_test_p2_plan and wfmh_test_base_plan): the cells of a job's rows against a brute-force
sum, the tiles of a block against its range, the single-tile rule, which instantiations of the packed kernel a block launches, the
order of the task list, the two rules by which a job leaves the tile phase, the geometry of the phase-2 rows, the kind of a base
job and the tiles of a wide one.  The expected values are worked out here, in Python, from the definitions."""
import ctypes as C
import random

import numpy as np
import pytest

from wfmash_amd import capi

NONE = 1 << 29   # SUB_NONE
BACK = 25        # RNG_BACK
P2K, P2ROWS = 32, 58
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def L():
    lib = capi.load()
    for name in ("wfmh_test_rows", "wfmh_test_tile_plan", "wfmh_test_p2_plan", "wfmh_test_base_plan"):
        assert name in capi.HOST_EXPORTS
        getattr(lib, name).restype = C.c_int
    lib.wfmh_test_rows.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.wfmh_test_tile_plan.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.wfmh_test_p2_plan.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_void_p]
    lib.wfmh_test_base_plan.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    return lib


def rows(L, queries):
    """queries: rows of (op, up to six arguments) -> int64 array (n, 2)"""
    q = np.zeros((len(queries), 7), dtype=np.int32)
    for i, row in enumerate(queries) if not isinstance(queries, np.ndarray) else ():
        q[i, :len(row)] = row
    if isinstance(queries, np.ndarray):
        q[:, :queries.shape[1]] = queries
    out = np.zeros((len(q), 2), dtype=np.int64)
    assert L.wfmh_test_rows(q.ctypes.data, len(q), out.ctypes.data) == 0
    return out


def rng_block(pl, tl, sub, s_from, s_to):
    return (max(-pl, -s_to, (tl - pl) - sub + s_from - BACK), min(tl, s_to, (tl - pl) + sub - s_from + BACK))


def tiles_for(Lo, R, core):
    return -(-(R - Lo + 1) // core) if R >= Lo else 0


def tile_plan(L, jobs, threads=512, Cc=2, T=100, chunk=2, core=None, reg=True, fine=True, coarse_on=False):
    """jobs: (pl, tl, sub, s0, mode, fine_s, packed, active) -> dict(threads_b, variants_b, core_c, tasks [(job, dir, tile, core)], n_pk)"""
    core = threads * Cc - 2 * T if core is None else core
    j = np.array(jobs, dtype=np.int32).reshape(-1, 8)
    rules = np.array([threads, Cc, T, chunk, core, reg, fine, coarse_on], dtype=np.int32)
    per_block = np.zeros(2 * chunk, dtype=np.int32)
    cap = 1 << 16
    tasks = np.zeros((cap, 4), dtype=np.int32)
    sc = np.zeros(3, dtype=np.int64)
    assert L.wfmh_test_tile_plan(j.ctypes.data, len(j), rules.ctypes.data, per_block.ctypes.data, tasks.ctypes.data, cap, sc.ctypes.data) == 0
    assert sc[1] <= cap
    return dict(threads_b=per_block[:chunk].tolist(), variants_b=per_block[chunk:].tolist(), core_c=int(sc[0]),
                tasks=[tuple(t) for t in tasks[:sc[1]].tolist()], n_pk=int(sc[2]), core=core)


def p2_plan(L, cand, i0=0, budget=1 << 40, threads=512, core=None):
    """cand: (pl, tl, sub, sf, sr, packed) -> dict(geo [(koff2, w2, nblk, p2_off, bm_off)], n, elems, bm_elems, maxw2, threads_c, core_c, tasks, n_pk)"""
    core = threads * 2 - 2 * P2K if core is None else core
    c = np.array(cand, dtype=np.int32).reshape(-1, 6)
    geo = np.zeros((len(c), 5), dtype=np.int64)
    cap = 1 << 16
    tasks = np.zeros((cap, 4), dtype=np.int32)
    sc = np.zeros(8, dtype=np.int64)
    assert L.wfmh_test_p2_plan(c.ctypes.data, len(c), i0, P2K, P2ROWS, budget, threads, core, geo.ctypes.data, tasks.ctypes.data, cap, sc.ctypes.data) == 0
    assert sc[6] <= cap
    return dict(geo=[tuple(g) for g in geo[:sc[0]].tolist()], n=int(sc[0]), elems=int(sc[1]), bm_elems=int(sc[2]), maxw2=int(sc[3]),
                threads_c=int(sc[4]), core_c=int(sc[5]), tasks=[tuple(t) for t in tasks[:sc[6]].tolist()], n_pk=int(sc[7]), core=core)


# ---- cells_sum ----

def _brute(pl, tl, sub, a, span):
    """sum over s = a .. a + span - 1 (span may be 0) of the cells of row s; arrays of one length"""
    width = int(span.max()) if len(span) else 0
    s = a[:, None] + np.arange(width, dtype=np.int64)[None, :]
    kinv = (tl - pl)[:, None]
    lo = np.maximum(np.maximum(-pl[:, None], -s), kinv - sub[:, None] + s)
    hi = np.minimum(np.minimum(tl[:, None], s), kinv + sub[:, None] - s)
    cells = np.maximum(0, hi - lo + 1)
    cells[np.arange(width)[None, :] >= span[:, None]] = 0
    return cells.sum(axis=1)


def test_cells_sum_small_grid(L):
    subs = np.array([0, 1, 2, 3, 5, 8, 13, 21, 40, NONE], dtype=np.int64)
    pl, tl, si, a, j = [x.ravel() for x in np.indices((15, 15, len(subs), 35, 38))]
    b = a - 1 + j
    keep = b <= 36
    pl, tl, si, a, b = pl[keep], tl[keep], si[keep], a[keep], b[keep]
    assert len(pl) == 15 * 15 * 10 * 735
    q = np.stack([np.zeros_like(pl), pl, tl, subs[si], a, b], axis=1)
    got = rows(L, q)[:, 0]
    exp = _brute(pl, tl, subs[si], a, b - a + 1)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (q[bad[0]].tolist(), int(got[bad[0]]), int(exp[bad[0]]))


def test_cells_sum_random(L):
    r = np.random.default_rng(0x7113)
    n = 20000
    pl, tl = r.integers(0, 3001, n), r.integers(0, 3001, n)
    sub = np.where(r.random(n) < 0.2, NONE, r.integers(0, 4001, n))
    a = r.integers(0, 2500, n)
    span = r.integers(0, 601, n)
    q = np.stack([np.zeros(n, dtype=np.int64), pl, tl, sub, a, a + span - 1], axis=1)
    got = rows(L, q)[:, 0]
    exp = _brute(pl, tl, sub, a, span)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (q[bad[0]].tolist(), int(got[bad[0]]), int(exp[bad[0]]))
    assert (exp > 0).sum() > n // 2


# ---- the tiles of a block ----

def _random_job(rng, bound=None):
    pl, tl = rng.randrange(1, 6000), rng.randrange(1, 6000)
    if bound is None:
        bound = rng.random() < 0.6
    sub = max(abs(tl - pl), rng.randrange(0, 3000)) if bound else NONE
    s0 = rng.choice([0, 0, 32, 100, 200]) + 100 * rng.randrange(0, 12)
    return pl, tl, sub, s0


def test_tiles_cover_every_block(L):
    rng = random.Random(0x711)
    blocks = []
    for _ in range(1500):
        pl, tl, sub, s0 = _random_job(rng)
        T, chunk, core = rng.choice([32, 100]), rng.choice([1, 2, 3]), rng.choice([64, 128, 312, 824, 960, 1024, rng.randrange(1, 1200)])
        for b in range(chunk):
            blocks.append((pl, tl, sub, s0 + b * T, s0 + (b + 1) * T, core))
    got = rows(L, [(1,) + bl[:5] for bl in blocks])
    queries, where = [], []
    for bl, (Lo, R) in zip(blocks, got.tolist()):
        assert (Lo, R) == rng_block(*bl[:5]), bl
        queries.append((3, Lo, R, bl[5]))
        where.append(len(queries))
        for idx in range(tiles_for(Lo, R, bl[5]) + 1):
            queries.append((2, Lo, R, idx, bl[5]))
    out = rows(L, queries).tolist()
    empty = 0
    for bl, (Lo, R), at in zip(blocks, got.tolist(), where):
        nt = out[at - 1][0]
        assert nt == tiles_for(Lo, R, bl[5]), (bl, nt)
        nxt = Lo
        for idx in range(nt):  # disjoint, in order, [L, R] exactly
            lo, hi = out[at + idx]
            assert lo == nxt and lo <= hi <= R and hi - lo + 1 <= bl[5], (bl, idx, lo, hi)
            assert hi - lo + 1 == bl[5] or idx == nt - 1
            nxt = hi + 1
        assert nxt == max(Lo, R + 1) if nt else R < Lo
        assert out[at + nt][0] > R, (bl, out[at + nt])  # one tile more would begin beyond the range
        empty += nt == 0
    assert 0 < empty < len(blocks) // 2


# ---- the single-tile rule ----

def _jobs_for_single_tile(rng, chunk, T):
    jobs = []
    for _ in range(rng.randrange(1, 9)):
        pl, tl = rng.randrange(50, 4000), rng.randrange(50, 4000)
        # (ranges that shrink within the chunk: a bound not far above the score the job stands at)
        s0 = T * rng.randrange(0, 700 // T)  # (ranges of up to 1500 diagonals: beyond one tile's 1024 as well)
        sub = rng.choice([NONE, max(abs(tl - pl), 2 * s0 + rng.randrange(-100, 400))])
        if rng.random() < 0.3:
            pl = tl = rng.randrange(20, 400)  # short problems: the range stops growing with the score
        jobs.append((pl, tl, sub, s0, 0, INT_MAX, rng.choice([0, 1]), int(rng.random() < 0.85)))
    return jobs


@pytest.mark.parametrize("T", [32, 100])
@pytest.mark.parametrize("chunk", [1, 2, 3])
def test_single_tile_fits_every_block(L, T, chunk):
    rng = random.Random(0x5171E + 7 * T + chunk)
    single = multi = shrinking = 0
    for _ in range(400):
        jobs = _jobs_for_single_tile(rng, chunk, T)
        fine = rng.random() < 0.7
        p = tile_plan(L, jobs, T=T, chunk=chunk, fine=fine)
        if p["core_c"] == p["core"]:
            multi += 1
            assert p["threads_b"] == [512] * chunk
            continue
        single += 1
        assert p["core_c"] == p["threads_b"][-1] * 2
        for i, (pl, tl, sub, s0, _, _, _, active) in enumerate(jobs):
            if not active:
                continue
            widths = []
            for b in range(chunk):
                Lo, R = rng_block(pl, tl, sub, s0 + b * T, s0 + (b + 1) * T)
                widths.append(R - Lo + 1)
                assert R - Lo + 1 <= p["threads_b"][b] * 2, (jobs[i], b, p)   # (both directions of the tile phase stand at s0: one range)
            shrinking += any(widths[b + 1] < widths[b] for b in range(chunk - 1))
            mine = [t for t in p["tasks"] if t[0] == i]
            assert mine == ([(i, 0, 0, p["core_c"]), (i, 1, 0, p["core_c"])] if max(widths) > 0 else []), (jobs[i], mine)
        assert all(t % 64 == 0 and 64 <= t <= 512 for t in p["threads_b"])
    assert single > 50 and multi > 10 and (chunk == 1 or shrinking > 0)


def test_single_tile_fits_phase2_rows(L):
    rng = random.Random(0x9271E)
    single = multi = 0
    for _ in range(600):
        cand = []
        for _ in range(rng.randrange(1, 7)):
            pl, tl = rng.randrange(50, 4000), rng.randrange(50, 4000)
            sf = rng.randrange(27, 700)
            sr = sf - rng.choice([0, 1])
            sub = rng.choice([NONE, max(abs(tl - pl), sf + sr + rng.randrange(0, 300))])
            if rng.random() < 0.3:
                pl = tl = rng.randrange(20, 400)
            cand.append((pl, tl, sub, sf, sr, rng.choice([0, 1])))
        p = p2_plan(L, cand)
        assert p["n"] == len(cand)
        if p["core_c"] == p["core"]:
            multi += 1
            assert p["threads_c"] == 512
            continue
        single += 1
        assert p["core_c"] == p["threads_c"] * 2 and p["threads_c"] % 64 == 0
        for i, (pl, tl, sub, sf, sr, _) in enumerate(cand):
            for d, sd in enumerate((sf, sr)):
                Lo, R = rng_block(pl, tl, sub, sd, sd + P2K)
                assert R - Lo + 1 <= p["threads_c"] * 2, (cand[i], d, p["threads_c"])
                assert [t for t in p["tasks"] if t[0] == i and t[1] == d] == ([(i, d, 0, p["core_c"])] if R >= Lo else [])
    assert single > 50 and multi > 50


# ---- variants_b: hand-derived ----

def test_variants_by_hand(L):
    wide = (3000, 3000)
    # a job the last chunk left in mode 5 (its meeting block runs again with per-score maxima) beside one that simply moves on
    p = tile_plan(L, [wide + (NONE, 200, 5, INT_MAX, 1, 1), wide + (NONE, 0, 0, INT_MAX, 1, 1)], coarse_on=True)
    assert p["variants_b"] == [3, 1]
    p = tile_plan(L, [wide + (NONE, 200, 5, INT_MAX, 1, 1)], coarse_on=True)
    assert p["variants_b"] == [2, 2]  # (block 1 of the job in mode 5: nothing asks for either form, FINE is launched)
    # a job that reaches its fine_s in block 1 of 2: scores 101 .. 200 stay below 250, 201 .. 300 do not
    assert tile_plan(L, [wide + (NONE, 100, 0, 250, 1, 1)], coarse_on=True)["variants_b"] == [1, 2]
    assert tile_plan(L, [wide + (NONE, 100, 0, 300, 1, 1)], coarse_on=True)["variants_b"] == [1, 2]
    assert tile_plan(L, [wide + (NONE, 100, 0, 301, 1, 1)], coarse_on=True)["variants_b"] == [1, 1]
    assert tile_plan(L, [wide + (NONE, 100, 0, 200, 1, 1)], coarse_on=True)["variants_b"] == [2, 2]
    assert tile_plan(L, [wide + (NONE, 100, 0, 0, 1, 1)], coarse_on=True, chunk=3)["variants_b"] == [2, 2, 2]
    # both kinds of job in one chunk; a job that is not active asks for nothing
    assert tile_plan(L, [wide + (NONE, 100, 0, 250, 1, 1), wide + (NONE, 0, 0, INT_MAX, 1, 1), wide + (NONE, 0, 0, 0, 1, 0)], coarse_on=True)["variants_b"] == [1, 3]
    # only jobs of the byte kernel: 2 everywhere
    assert tile_plan(L, [wide + (NONE, 100, 0, 250, 0, 1), wide + (NONE, 0, 5, INT_MAX, 0, 1)], coarse_on=True)["variants_b"] == [2, 2]
    # coarse maxima off: 2 everywhere, whatever the jobs
    assert tile_plan(L, [wide + (NONE, 100, 0, 250, 1, 1), wide + (NONE, 0, 0, INT_MAX, 1, 1)], coarse_on=False)["variants_b"] == [2, 2]


# ---- the order of the task list ----

def test_task_order(L):
    rng = random.Random(0x7A5C)
    several = 0
    for _ in range(300):
        T, chunk = rng.choice([32, 100]), rng.choice([1, 2, 3])
        threads = rng.choice([64, 128, 512])
        jobs = []
        for _ in range(rng.randrange(1, 10)):
            pl, tl, sub, s0 = _random_job(rng)
            jobs.append((pl, tl, sub, s0, 0, INT_MAX, rng.choice([0, 0, 1, 3]), int(rng.random() < 0.8)))
        p = tile_plan(L, jobs, threads=threads, T=T, chunk=chunk, core=max(8, threads * 2 - 2 * T))
        exp = {True: [], False: []}
        for i, (pl, tl, sub, s0, _, _, packed, active) in enumerate(jobs):
            if not active:
                continue
            nt = max(tiles_for(*rng_block(pl, tl, sub, s0 + b * T, s0 + (b + 1) * T), p["core_c"]) for b in range(chunk))
            several += nt > 1
            exp[packed != 0] += [(i, d, t, p["core_c"]) for d in (0, 1) for t in range(nt)]
        assert p["tasks"] == exp[True] + exp[False]
        assert p["n_pk"] == len(exp[True])
    assert several > 100


# ---- tile_job_leaves ----

def test_tile_job_leaves_at_the_edges(L):
    big = (5000, 5000)
    q = []
    for op, T in ((4, 100), (5, 32)):
        for chunk in (1, 2, 3):
            s0 = 3 * T
            q += [(op,) + big + (NONE, s0, s0 + chunk * T + 2, chunk),   # the chunk's last score (and two) still fit the band: stays
                  (op,) + big + (NONE, s0, s0 + chunk * T + 1, chunk),   # one short: leaves
                  (op,) + big + (NONE, s0, 0, chunk)]                    # no band
    out = rows(L, q)[:, 0].tolist()
    assert out == [0, 1, 0] * 6
    q = [(4,) + big + (1000, 564, 0, 2),     # 2 s0 = bound + 128: stays
         (4,) + big + (1000, 565, 0, 2),     # past half the bound (+ 64): leaves
         (4,) + big + (10, 35, 0, 2),        # the bound as it stood 25 scores ago leaves diagonal 0: stays
         (4,) + big + (10, 36, 0, 2),        # nothing left within the bound: leaves
         (4,) + big + (NONE, 10**6, 0, 2),   # no bound
         (4,) + big + (1000, 565, 10**6, 2), # a wide band does not keep it
         (4,) + big + (1000, 100, 301, 2)]   # a bound that holds does not keep it either: the band's rule
    assert rows(L, q)[:, 0].tolist() == [0, 1, 0, 1, 0, 1, 1]
    assert rng_block(5000, 5000, 10, 35, 135) == (0, 0) and rng_block(5000, 5000, 10, 36, 136) == (1, -1)


# ---- the geometry of the phase-2 rows ----

def test_p2_geometry_and_budget(L):
    rng = random.Random(0x9262)
    cand = []
    for _ in range(400):
        pl, tl = rng.randrange(1, 6000), rng.randrange(1, 6000)
        sf = rng.randrange(27, 3000)
        sr = sf - rng.choice([0, 1])
        if min(sf, sr) < 27:
            sr = sf
        sub = rng.choice([NONE, max(abs(tl - pl), sf + sr + rng.randrange(0, 300))])
        cand.append((pl, tl, sub, sf, sr, rng.choice([0, 1])))
    p = p2_plan(L, cand)
    assert p["n"] == len(cand)
    off = bm = 0
    for (pl, tl, sub, sf, sr, _), (koff2, w2, nblk, p2_off, bm_off) in zip(cand, p["geo"]):
        Lo, R = rng_block(pl, tl, sub, min(sf, sr) - 27, max(sf, sr) + P2K)
        assert koff2 % 4 == 0 and w2 % 4 == 0 and nblk == (w2 >> 6) + 1
        if R >= Lo:
            assert Lo + koff2 >= 4 and 0 <= Lo + koff2 <= R + koff2 < w2, (pl, tl, sub, sf, sr, koff2, w2)
        assert (p2_off, bm_off) == (off, bm)
        off += w2 * 2 * 5 * P2K
        bm += nblk * 2 * P2ROWS * 5
    assert (p["elems"], p["bm_elems"], p["maxw2"]) == (off, bm, max(g[1] for g in p["geo"]))
    # a job that stands below score 27: the window begins at score 0
    g = p2_plan(L, [(300, 300, 40, 5, 4, 1)])["geo"][0]
    Lo, R = rng_block(300, 300, 40, 0, 5 + P2K)
    assert g[0] % 4 == 0 and Lo + g[0] >= 4 and R + g[0] < g[1]
    # the budget cuts the list into chunks, none of them empty; a chunk of several jobs fits it
    for budget in (1, 1 << 20, 8 << 20, 64 << 20):
        i0, chunks = 0, 0
        while i0 < len(cand):
            c = p2_plan(L, cand, i0=i0, budget=budget)
            assert c["n"] >= 1
            assert c["n"] == 1 or (c["elems"] + 2 * c["bm_elems"]) * 4 <= budget
            assert [g[1:3] for g in c["geo"]] == [g[1:3] for g in p["geo"][i0:i0 + c["n"]]] and c["geo"][0][3:] == (0, 0)
            assert {t[0] for t in c["tasks"]} <= set(range(c["n"]))
            if i0 + c["n"] < len(cand):  # it stopped because the next job did not fit
                nxt = p["geo"][i0 + c["n"]]
                assert (c["elems"] + nxt[1] * 2 * 5 * P2K + 2 * (c["bm_elems"] + nxt[2] * 2 * P2ROWS * 5)) * 4 > budget
            i0 += c["n"]
            chunks += 1
        assert chunks == len(cand) if budget == 1 else chunks >= 1
    assert p2_plan(L, cand, budget=64 << 20)["n"] > 1


# ---- base jobs ----

def base_kind(L, width, pl=500, tl=500, tries=0, acgt=True, base_v2=True, base_tiles=True, force_tiles=False, jobs=1000):
    q = np.array([width, pl, tl, tries, acgt, base_v2, base_tiles, force_tiles, jobs < 128, 512 if jobs < 128 else 2048], dtype=np.int32)
    out = np.zeros(1, dtype=np.int32)
    assert L.wfmh_test_base_plan(0, q.ctypes.data, 1, out.ctypes.data) == 0
    return int(out[0])


def test_base_kind(L):
    k = lambda *a, **kw: base_kind(L, *a, **kw)
    # the register kernel's three widths, the tiles beyond them
    assert [k(w) for w in (1, 128, 129, 640, 641, 2048, 2049, 9000)] == [0, 0, 1, 1, 2, 2, 5, 5]
    assert k(2049, base_tiles=False) == 4 and k(2048, base_tiles=False) == 2
    # an N or lower case: the ring kernel, 1024 threads beyond 2048 diagonals -- beyond 512 when the call has fewer than 128 jobs
    assert [k(w, acgt=False) for w in (128, 512, 513, 2048, 2049)] == [3, 3, 3, 3, 4]
    assert [k(w, acgt=False, jobs=127) for w in (512, 513, 2049)] == [3, 4, 4]
    assert [k(w, acgt=False, jobs=128) for w in (512, 513, 2048, 2049)] == [3, 3, 3, 4]
    # a few jobs: retries and rows beyond 640 go to the tiles
    assert [k(w, jobs=127) for w in (128, 129, 640, 641, 2048, 2049)] == [0, 1, 1, 5, 5, 5]
    assert [k(w, jobs=127, tries=1) for w in (128, 129, 640, 641)] == [0, 5, 5, 5]
    assert [k(w, jobs=128, tries=1) for w in (128, 129, 640, 641, 2048)] == [0, 1, 1, 2, 2]
    assert [k(w, jobs=127, tries=1, base_tiles=False) for w in (129, 641, 2049)] == [1, 2, 4]
    # WFM_BASE_TILES=2: everything beyond 128 diagonals
    assert [k(w, force_tiles=True) for w in (128, 129, 2049)] == [0, 5, 5]
    # jobs without a cell ride with kind 1; other penalties or WFM_BASE_V2=0: the ring kernel takes everything
    assert k(0, pl=0) == 1 and k(0, tl=0, acgt=False) == 1 and k(0, pl=0, base_v2=False) == 3
    assert [k(w, base_v2=False) for w in (100, 2048, 2049)] == [3, 3, 4]
    assert {k(w, acgt=a) for w in (100, 600, 2000, 3000) for a in (True, False)} == {0, 1, 2, 3, 4, 5}


def test_base_tiles_cover_width_and_budget(L):
    rng = random.Random(0xBA5E)
    for _ in range(200):
        T = rng.choice([5, 50, 125, 400])
        n = rng.randrange(1, 12)
        jobs = [(rng.randrange(1, 12000), rng.randrange(1, 9000)) for _ in range(n)]
        q = np.array([T, 512] + [x for j in jobs for x in j], dtype=np.int32)
        out = np.zeros(2 + n, dtype=np.int32)
        assert L.wfmh_test_base_plan(1, q.ctypes.data, n, out.ctypes.data) == 0
        core, nblocks = int(out[0]), int(out[1])
        assert core == 1024 - 2 * T  # two diagonals per lane, T columns of halo on either side
        for (w, _), nt in zip(jobs, out[2:].tolist()):
            assert (nt - 1) * core < w <= nt * core
        smax = max(s for _, s in jobs)
        assert (nblocks - 2) * T < smax <= (nblocks - 1) * T  # row 0 and smax rows
