"""Long records under a device-memory budget their full wavefront rings do not fit: the rings grow with the score a job
reaches (bands b, 4 b, 16 b ...), a tiled job that simply ran out of its band keeps its snapshot, has it widened
(wfa_ring_widen_kernel) and goes on from there, everybody else starts again from score 0 on the grown band.  Memory
follows the alignment's score, not the record's length.

Every case runs on a handle of its own under WFM_MEM_BUDGET_MB and is held against the CPU oracle."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

WFM_PF_RING_GROWN = 256
WFM_ST_OOM = -200
TILE_T, TILE_CHUNK = 100, 2  # TileCfg's defaults: scores per tile block, blocks between two looks of the host


def _pairs(seed, n, lens, rates):
    import random
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = rng.choice(lens)
        p = synth.random_dna(seed * 1000 + i, L)
        t = synth.mutate(p, rng.choice(rates), seed * 7919 + i) if L else b""
        r = rng.random()
        if r < 0.08:
            t = synth.random_dna(seed * 31 + i, rng.randrange(0, 400))
        elif r < 0.12:
            t = b""
        elif r < 0.16:
            p = b""
        out.append((p, t))
    return out


def _check_batch(gpu, oracle, items, pen=None):
    """status 0, a CIGAR that spells both sequences, its score the reported score and the oracle's, op strings identical."""
    res = gpu.align(items, pen)
    for it, r in zip(items, res):
        print(f"problem {len(it[0])} x {len(it[1])}: status {r.status} score {r.score} cells {r.cells}")
    ops_o, sc_o, _, failed = oracle.align_batch_biwfa([it[0] for it in items], [it[1] for it in items], pen)
    assert failed == 0
    n_bad = 0
    for it, r, oo, so in zip(items, res, ops_o, sc_o):
        p, t = it[0], it[1]
        assert r.status == 0, (len(p), len(t), r.status)
        assert oracle.ops_check(r.ops, p, t) == 0
        assert oracle.ops_score(r.ops, pen) == r.score == int(so)
        if r.ops != oo:
            n_bad += 1
    assert n_bad == 0, f"{n_bad}/{len(items)} CIGARs differ from the oracle"
    return res


def _balanced(seed, length, rate, n):
    """n pairs of `length` bases, `rate` substitutions and short indels, |tl - pl| < 64 (no score bound is asked for such a
    root): the first mutation seeds from `seed` on that leave the lengths that close."""
    out = []
    s = seed
    while len(out) < n:
        p = synth.random_dna(s, length)
        t = synth.mutate(p, rate, s + 0x10000)
        s += 1
        if abs(len(t) - len(p)) < 64:
            out.append((p, t))
    return out


def _grown_line(err):
    """(jobs, widened and resumed, started again, largest band) of the last `grown rings` line, or None."""
    m = re.findall(r"grown rings: (\d+) jobs, (\d+) widened and resumed, (\d+) started again, largest band (\d+)", err)
    return tuple(int(x) for x in m[-1]) if m else None


def _handle(monkeypatch, budget_mb, **env):
    monkeypatch.setenv("WFM_DEBUG", os.environ.get("WFM_DEBUG") or "1")
    if budget_mb is not None:
        monkeypatch.setenv("WFM_MEM_BUDGET_MB", str(budget_mb))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return capi.Handle(0)


def test_balanced_root_past_its_band_resumes_on_a_wider_ring(oracle, monkeypatch, capfd):
    """80 kbp at 4 % under 128 MB: the root's guessed band (4312 scores a direction) is spent near half of what each direction
    needs, the full ring (160 k columns x 1280 B = 205 MB) does not fit.  The snapshot at the band's last block boundary is
    widened into a ring for 4 x 4312 scores and the tile phase goes on from there."""
    items = _balanced(0x1001, 80_000, 0.04, 3)
    h = _handle(monkeypatch, 128)
    try:
        _check_batch(h, oracle, items)
        flags = h.problem_flags(len(items))
    finally:
        h.close()
    err = capfd.readouterr().err
    assert all(int(f) & WFM_PF_RING_GROWN for f in flags), flags
    assert all(int(f) & capi.WFM_PF_ROOT_AGAIN for f in flags), flags
    g = _grown_line(err)
    assert g is not None, err[-2000:]
    assert g[1] >= 1, g


def test_the_rings_the_driver_used_are_the_planner_s(oracle, monkeypatch, capfd):
    """One pair of the case above: every grown ring the level driver reports -- band, columns, tile kernels or step kernel alone --
    is what plan_ring (csrc/wfa_plan.h, held on a CPU by tests/test_ring_plan_cpu.py) gives for that job: a root of 80 000 x its
    text under 128 MiB that has spent the band it had before (the guessed 4312 at first, then the band of its last grown ring;
    the same input once more where a resumed job is sent back to score 0 on the band it has)."""
    items = _balanced(0x1001, 80_000, 0.04, 1)
    h = _handle(monkeypatch, 128)
    try:
        _check_batch(h, oracle, items)
    finally:
        h.close()
    err = capfd.readouterr().err
    lines = re.findall(r"\[wfm\] grown ring: problem (\d+), (\w+) of (\d+) x (\d+): band (\d+), (\d+) columns on the (tile kernels|step kernel alone)", err)
    assert lines, err[-2000:]
    had, handed = 4096 + TILE_CHUNK * TILE_T + 16, None  # the band of the job's last ring; the band the planner was last handed
    for prob, kind, pl, tl, band, cols, kernel in lines:
        print(f"grown ring: {kind} {pl} x {tl}: band {band}, {cols} columns on the {kernel}; the band it had: {had}")
        assert (int(prob), kind, int(pl), int(tl)) == (0, "root", 80_000, len(items[0][1]))
        before = handed if int(band) == had else had
        p = capi.ring_plan(int(pl), int(tl), 128 << 20, noband=1, band=before, use_band=True, over_budget=True)
        assert p is not None and p["grown"], (before, p)
        assert (p["band"], p["width"], p["tile_it"]) == (int(band), int(cols), kernel == "tile kernels"), (before, p)
        had, handed = int(band), before


def test_a_resumed_job_that_meets_next_to_its_snapshot_starts_again(oracle, monkeypatch, capfd):
    """A snapshot holds the gap components only as deep as the next tile block loads them; a resumed job whose directions meet
    within 26 scores of it would hand rows on that are not there, and runs again from score 0 on the same band.  Forced here for
    every resumed job (WFM_RESUME_MARGIN): the pairs of the case above, the same CIGARs."""
    items = _balanced(0x1001, 80_000, 0.04, 2)
    h = _handle(monkeypatch, 128, WFM_RESUME_MARGIN="1000000")
    try:
        _check_batch(h, oracle, items)
        flags = h.problem_flags(len(items))
    finally:
        h.close()
    err = capfd.readouterr().err
    assert all(int(f) & WFM_PF_RING_GROWN for f in flags), flags
    g = _grown_line(err)
    assert g is not None and g[1] >= 2 and g[2] >= 2 and g[3] == 4 * (4096 + TILE_CHUNK * TILE_T + 16), (g, err[-2000:])


def test_too_small_a_hint_on_cut_rows_starts_again_on_a_grown_band(oracle, monkeypatch, capfd):
    """80 kbp against 82 kbp (one insertion of 2 kbp) with a score hint of 3000: the root runs under the guess, its rows are cut
    to what could stay below it -- no state of the unbounded problem -- so after the guess has failed the job starts again from
    score 0, on a band grown from the one it had.

    Divergence beside the insertion: 1.5 %, not the 4 % of the other cases.  The band after the failed guess is
    max(4 x 1844, 4096) = 7376 scores a direction; at 4 % a direction needs ~11 k, so that band runs out as well -- unbounded
    this time, a plain band exit, which by the rules resumes on a widened ring, and the case asks for a run that only starts
    again.  At 1.5 % (score ~10 k, 5 k a direction) the first grown band holds.  The hint, the lengths and the insertion stay."""
    items = []
    for i in range(2):
        p = synth.random_dna(0x2001 + i, 80_000)
        t = synth.mutate(p, 0.015, 0x2101 + i)
        t = t[:40_000] + synth.random_dna(0x2201 + i, 2_000 + len(p) - len(t)) + t[40_000:]
        assert len(t) == len(p) + 2_000
        items.append((p, t, capi.WFM_MODE_END2END_BIWFA, 0, 0, 0, 0, 3000))
    h = _handle(monkeypatch, 128)
    try:
        _check_batch(h, oracle, items)
        flags = h.problem_flags(len(items))
    finally:
        h.close()
    err = capfd.readouterr().err
    assert all(int(f) & WFM_PF_RING_GROWN for f in flags), flags
    assert "ran past their hint" in err, err[-2000:]
    g = _grown_line(err)
    assert g is not None, err[-2000:]
    assert g[2] >= 1 and g[1] == 0, g


def test_penalties_without_tiles_get_a_narrow_ring(oracle, monkeypatch, capfd):
    """Scope 102: the tile kernels do not take the job, its rings are 128 rows deep (60 k columns x 5120 B = 307 MB for 30 kbp
    a side).  Under 64 MB the step kernel runs it alone on a ring for WFM_BAND_ROOT scores a direction."""
    pen = (5, 8, 2, 100, 1)
    items = _balanced(0x3001, 30_000, 0.03, 2)
    h = _handle(monkeypatch, 64)
    try:
        _check_batch(h, oracle, items, pen=pen)
        flags = h.problem_flags(len(items))
    finally:
        h.close()
    err = capfd.readouterr().err
    assert all(int(f) & WFM_PF_RING_GROWN for f in flags), flags
    g = _grown_line(err)
    assert g is not None and g[0] >= 2 and g[1] == 0, (g, err[-2000:])


def _chunk_cells(pl, tl, s0):
    """Cells of one chunk of tile blocks from score s0 on, both directions: a row of score s spans [max(-pl, -s), min(tl, s)]."""
    n = 0
    for s in range(s0 + 1, s0 + TILE_CHUNK * TILE_T + 1):
        n += 2 * (min(tl, s) - max(-pl, -s) + 1)
    return n


def test_nothing_is_recomputed_on_the_resume_path(oracle, monkeypatch, capfd):
    """The pairs of the first case on full rings (512 MB, WFM_BAND=0) and under 128 MB.  A job leaves its band BEFORE the chunk of
    blocks that would not fit and goes on from that very snapshot, so the resumed run computes what the run on a full ring
    computes: the cells may differ by no more than one chunk of blocks at the resume point (band 4312: chunks of 2 x 100
    scores start at 0, 200 ... 4000, the one from s0 = 4200 would pass the band).  Held per problem for
    wfm_result_t::cells -- the step and base kernels' cells of a problem -- and for the call for
    wfm_stats_t::cells_tile_unique, the tile kernels' cells from where a pass starts to where it leaves its jobs, which is
    where a job that started again would show: the cells up to s0, (4200 / 8000)^2 or a quarter of the whole.  (The call's
    total, wfm_stats_t::cells, is printed and not held: it also counts the blocks the tile kernels run twice, and which blocks
    those are differs between children on full rings without a third ring and children on narrow rings with one,
    TileJob::ring_prev -- no recomputation of this path.)"""
    items = _balanced(0x1001, 80_000, 0.04, 3)
    runs = {}
    for mb, env in ((512, {"WFM_BAND": "0"}), (128, {})):
        monkeypatch.delenv("WFM_BAND", raising=False)
        h = _handle(monkeypatch, mb, **env)
        try:
            res = h.align(items)
            st = h.stats()
            runs[mb] = ([r.cells for r in res], int(st.cells_tile_unique), [r.ops for r in res], [r.status for r in res], int(st.cells))
        finally:
            h.close()
    err = capfd.readouterr().err
    assert runs[512][3] == [0, 0, 0] and runs[128][3] == [0, 0, 0], (runs[512][3], runs[128][3])
    assert runs[512][2] == runs[128][2]
    g = _grown_line(err)
    assert g is not None and g[1] >= 1, (g, err[-2000:])
    band = 4096 + TILE_CHUNK * TILE_T + 16
    step = TILE_CHUNK * TILE_T
    s0 = ((band - step - 2) // step + 1) * step  # the first chunk start whose last score does not fit the band
    total_allow = 0
    for (p, t), c_full, c_narrow in zip(items, runs[512][0], runs[128][0]):
        allow = _chunk_cells(len(p), len(t), s0)
        total_allow += allow
        print(f"step + base kernel cells per problem: full ring {c_full}, grown rings {c_narrow}, allowance {allow}")
        assert c_narrow - c_full <= allow, (c_full, c_narrow, allow)
    print(f"tile cells in the result: full rings {runs[512][1]}, grown rings {runs[128][1]}, allowance {total_allow}")
    print(f"all cells of the call: full rings {runs[512][4]}, grown rings {runs[128][4]}")
    assert runs[128][1] - runs[512][1] <= total_allow, (runs[512][1], runs[128][1], total_allow)


def test_the_ordinary_retry_path_is_untouched(oracle, monkeypatch, capfd):
    """Full rings fit (96 MB, records of 9 - 14 kbp): jobs that run out of their band go to full rings as ever, nothing grows."""
    h = _handle(monkeypatch, 96, WFM_BAND_ROOT="200", WFM_OVERLAP="0")
    try:
        items = _pairs(31, 40, [9000, 14000], [0.002, 0.01, 0.04])
        _check_batch(h, oracle, items)
        flags = h.problem_flags(len(items))
    finally:
        h.close()
    err = capfd.readouterr().err
    assert not any(int(f) & WFM_PF_RING_GROWN for f in flags), flags
    assert "grown rings" not in err
    lines = [l for l in err.splitlines() if "narrow rings" in l]
    assert lines, err[-1500:]
    jobs, retried = (int(x) for x in re.search(r"narrow rings: (\d+) jobs, (\d+) ran out", lines[-1]).groups())
    assert jobs > 0 and retried > 0, lines[-1]


def _align_rc(h, items):
    """Handle.align that also returns wfm_align_batch's own return value (the number of problems that failed)."""
    probs, keep, n = capi._make_problems(items)
    pn = capi.Penalties(*capi.DEFAULT_PEN)
    nbytes = h._L.wfm_align_arena_bytes(probs, n)
    arena = np.zeros(nbytes + 8, dtype=np.uint8)
    res = (capi.Result * max(n, 1))()
    rc = h._L.wfm_align_batch(h._p, C.byref(pn), probs, n, res, arena.ctypes.data, nbytes)
    out = []
    for i in range(n):
        r = res[i]
        out.append((r.status, r.score, arena[r.ops_off:r.ops_off + r.ops_len].tobytes() if r.status == 0 else None))
    return rc, out


def test_a_score_beyond_the_budget_fails_cleanly(oracle, monkeypatch):
    """80 kbp at 25 % under 16 MB: band 4312 (11 MB, step kernel) is spent, the next band is clamped to the ~6 k scores the budget
    holds and is spent too -> WFM_ST_OOM for that problem alone, set by the host before anything is launched for it."""
    p = synth.random_dna(0x6001, 80_000)
    long_pair = (p, synth.mutate(p, 0.25, 0x6002))
    q = synth.random_dna(0x6003, 3_000)
    short_pair = (q, synth.mutate(q, 0.05, 0x6004))
    h = _handle(monkeypatch, 16)
    try:
        rc, res = _align_rc(h, [long_pair, short_pair])
        print("call returned", rc, "statuses", [r[0] for r in res])
        assert rc == 1
        assert res[0][0] == WFM_ST_OOM
        rco, ops, sc, _ = oracle.align_biwfa(*short_pair)
        assert rco == 0 and res[1][0] == 0 and res[1][1] == sc and res[1][2] == ops
        _check_batch(h, oracle, [short_pair])  # the handle goes on working
    finally:
        h.close()


def _write_case(tmp_path, name, rate, seed):
    p = synth.random_dna(seed, 80_000)
    q = synth.mutate(p, rate, seed + 1)
    recs = [("tgt", p), ("qry", q)]
    fa = str(tmp_path / f"{name}.fa")
    synth.write_fasta(fa, recs)
    m = str(tmp_path / f"{name}.map.paf")
    row = "\t".join(map(str, ["qry", len(q), 0, len(q), "+", "tgt", len(p), 0, len(p), 100, len(p), 30, "id:f:0.99", "kc:f:0.9"]))
    with open(m, "w") as f:
        f.write(row + "\n")
    return fa, m, row, dict(recs)


def test_through_the_align_driver(monkeypatch, tmp_path, capfd):
    """A mapping row that claims 99 % identity for a pair 5 % apart: the driver's hint (~6 k) is far below the ~21 k the pair costs.
    Under 128 MB the record is written all the same, equal to the host oracle's; a pair 25 % apart under 16 MB is dropped, with a
    warning on stderr."""
    from oracle import wflign_host as W
    fa, m, row, seqs = _write_case(tmp_path, "a", 0.05, 0x7001)
    out = str(tmp_path / "a.paf")
    h = _handle(monkeypatch, 128)
    try:
        capi.align_paf(h, fa, m, out)
    finally:
        h.close()
    got = [l.rstrip("\n") for l in open(out)]
    print("records written:", len(got))
    want = W.align_mapping_lines([row], seqs, seqs)
    assert len(want) == 1
    assert got == want
    capfd.readouterr()

    fa, m, row, seqs = _write_case(tmp_path, "b", 0.25, 0x7101)
    out = str(tmp_path / "b.paf")
    h = _handle(monkeypatch, 16)
    try:
        capi.align_paf(h, fa, m, out)
    finally:
        h.close()
    err = capfd.readouterr().err
    assert open(out).read() == ""
    warn = [l for l in err.splitlines() if l.startswith("[wfmash] WARNING: qry:")]
    assert warn and "-> tgt:" in warn[0] and warn[0].endswith("not aligned: its wavefronts do not fit the device memory budget"), err[-2000:]


def _planted_pair(n, n_sub, n_indel, seed):
    """A random sequence of n bases and a copy with n_sub substitutions, n_indel 1-base insertions and as many 1-base deletions
    at distinct, well separated positions (equal lengths).  Returns (pattern, text, cost of the planted script)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    code = rng.integers(0, 4, n, dtype=np.uint8)
    n_ev = n_sub + 2 * n_indel
    pos = np.sort(rng.choice(n // 8 - 2, n_ev, replace=False).astype(np.int64) * 8 + 4)  # at least 8 bases apart
    kind = rng.permutation(np.concatenate([np.zeros(n_sub, np.int8), np.ones(n_indel, np.int8), np.full(n_indel, 2, np.int8)]))
    tcode = code.copy()
    sub = pos[kind == 0]
    tcode[sub] = (code[sub] + rng.integers(1, 4, len(sub), dtype=np.uint8)) & 3
    keep = np.ones(n, dtype=bool)
    keep[pos[kind == 2]] = False                               # deletions
    reps = np.ones(n, dtype=np.int64)
    reps[pos[kind == 1]] = 2                                   # insertions: the base once more (any base costs the same)
    reps[~keep] = 0
    t = np.repeat(tcode, reps)
    assert len(t) == n
    return acgt[code].tobytes(), acgt[t].tobytes(), 5 * n_sub + 10 * 2 * n_indel


def test_full_size_record_at_the_default_budget(oracle, monkeypatch, capfd):
    """One pair of 14 Mbp a side: a full ring would be 28 M columns x 1280 B = 35.8 GB, above the 32 GB cap of any handle.  No
    oracle holds this: the CIGAR must spell both sequences, score what is reported, and cost no more than the planted script."""
    p, t, cost = _planted_pair(14_000_000, 14_000, 7_000, 0x8001)
    monkeypatch.delenv("WFM_MEM_BUDGET_MB", raising=False)
    h = _handle(monkeypatch, None)
    try:
        t0 = time.time()
        r = h.align([(p, t)])[0]
        dt = time.time() - t0
        flags = h.problem_flags(1)
        st = h.stats()
        print(f"14 Mbp pair: status {r.status} score {r.score} (planted {cost}) in {dt:.1f} s, cells {st.cells}, device ms {st.ms_kernels:.1f}")
    finally:
        h.close()
    err = capfd.readouterr().err
    print("\n".join(l for l in err.splitlines() if "grown rings" in l or "narrow rings" in l))
    assert r.status == 0
    assert oracle.ops_check(r.ops, p, t) == 0
    assert oracle.ops_score(r.ops) == r.score
    assert r.score <= cost
    assert int(flags[0]) & WFM_PF_RING_GROWN
