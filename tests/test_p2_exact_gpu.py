"""The exact walk of phase 2 on the GPU (WFM_P2_EXACT; P2Job::exact, wfa_p2_exact_kernel): a job that left the tile phase at the end planned from
its known score looks only at the pairs of rows of exactly that score -- no maxima, no list of pairs -- and every record must come out as before.

The pairs of tests/test_p2_exact_cpu.py (about 4000 bases: planned_meet_cases.select(100), select(32), gap_pairs(), the short gaps that put a
child's breakpoint into I1 / D1), two pairs of 12 kb at 10 % (rows past 1024 diagonals: several strides of the workgroup over a row), and the
roots of tests/reuse_touch_cases.py (long two-piece gaps: hits 24 and more tests behind the planned end).  They run through wfm_align_batch
under the configurations of MACHINE with WFM_P2_EXACT = 1 and = 0 in one process: status, score and op string of every record equal
oracle.align_biwfa's and the other form's.  That the path ran is read from wfm_get_tile_counters: p2_exact >= the jobs below the roots in the
oracle's recursion (every one of them takes its planned end), 0 with the switch off and for pairs with an N (the byte kernel's jobs search),
p2_exact_misses == 0 everywhere but under WFM_P2_EXACT_REACH = 1, where every job whose hit lies behind its first test misses and goes
through the search from the same state.  Record tags: no more records whose overlap walk needed a second round of rows than with the switch off.
"""
import functools
import re

import pytest

import p2_exact_cases as XC
import planned_meet_cases as PM
import reuse_touch_cases as RT
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

ENV_KEYS = ("WFM_TILE", "WFM_TILE_T", "WFM_TILE_THREADS", "WFM_TILE_COARSE", "WFM_TILE_COARSE_MIN_BLOCKS", "WFM_TILE_COARSE_MAX_JOBS", "WFM_TILE_RING3",
            "WFM_TILE_FINE", "WFM_TILE_CHUNK", "WFM_TILE_EXACT", "WFM_TILE_FINE_MARGIN", "WFM_P2", "WFM_REUSE", "WFM_REUSE_EVERY", "WFM_REUSE_MIN_BLOCKS",
            "WFM_TILE_PLANNED_END", "WFM_TILE_PLANNED_DEEP", "WFM_SUB_SLACK", "WFM_P2_EXACT", "WFM_P2_EXACT_REACH", "WFM_MEM_BUDGET_MB")


def _n_twin(p, t):
    """the pair with one N at the same place of both sequences, where they agree and the eight bases around agree too: the byte kernels"""
    pos = next(q for q in range(150, 400) if p[q - 8:q + 8] == t[q - 8:q + 8])
    return p[:pos] + b"N" + p[pos + 1:], t[:pos] + b"N" + t[pos + 1:]


@functools.lru_cache(maxsize=None)
def _set(name):
    """-> (items, oracle ops, oracle scores, jobs below the roots in the oracle's recursion): computed once, shared, never changed"""
    from oracle import pyoracle as O
    ordinary = list(PM.select(100)) + list(PM.select(32)) + list(PM.gap_pairs()) + XC.short_gap_pairs() + XC.long_pairs()
    twins = [_n_twin(*PM.select(100)[q]) for q in (0, 5)]
    if name == "n":
        items, exact = twins, []
    elif name == "mixed":
        items, exact = twins + ordinary[:6], ordinary[:6]
    elif name == "touch":
        items, exact = [(r.p, r.t) for r in RT.roots() if not r.spec.n_at], []   # (their recursion is tests/test_p2_exact_cpu.py's: not walked again here)
    else:
        items = exact = ordinary
    ops, scores, _, failed = O.align_batch_biwfa([p for p, _ in items], [t for _, t in items], None)
    assert failed == 0
    below = sum(len(PM.descendants(p, t)) for p, t in exact)   # (the children of a pair with an N run on the byte kernel: they search)
    return items, ops, [int(s) for s in scores], below


P2_LINE = re.compile(r"phase 2 from rows computed ahead: (\d+) jobs.*exact walk ([0-9.]+) % of the jobs, missed ([0-9.]+) %")


def _run(monkeypatch, capfd, env, name):
    """one align call on a fresh handle under `env` -> (records, tile counters, records tagged with a second round of rows, (jobs, share of the
    exact walk) of every chunk of phase 2); every record checked against the oracle"""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("WFM_DEBUG", "1")
    items, ops, scores, _ = _set(name)
    capfd.readouterr()
    h = capi.Handle(0)
    try:
        res = h.align(items)
        ctr, flags = h.tile_counters(), h.problem_flags(len(items))
    finally:
        h.close()
    err = capfd.readouterr().err
    bad = [(i, r.status, r.score, scores[i]) for i, r in enumerate(res) if r.status != 0 or r.score != scores[i] or r.ops != ops[i]]
    assert not bad, (env, name, bad[:8], len(bad))
    chunks = [(int(n), float(x)) for n, x, _ in P2_LINE.findall(err)]
    assert chunks, err[-2000:]
    # the lines add up to the call's counter
    assert abs(sum(n * x / 100.0 for n, x in chunks) - ctr["p2_exact"]) <= 0.0005 * sum(n for n, _ in chunks) + 0.01, (chunks, ctr)   # (shares are printed to 0.1 %)
    return [(r.status, r.score, r.ops) for r in res], ctr, sum(1 for f in flags if int(f) & capi.WFM_PF_P2_ROUNDS), chunks


def _both(monkeypatch, capfd, env, name, again=False):
    """the switch on and off (and, `again`, on once more: the default, read per call) in one process -> counters of on and off, chunks of on"""
    on, ctr_on, rounds_on, chunks = _run(monkeypatch, capfd, dict(env, WFM_P2_EXACT="1"), name)
    off, ctr_off, rounds_off, _ = _run(monkeypatch, capfd, dict(env, WFM_P2_EXACT="0"), name)
    assert on == off
    if again:
        third, ctr_again, _, _ = _run(monkeypatch, capfd, env, name)
        assert third == on and ctr_again == ctr_on, (ctr_on, ctr_again)
    print("on ", ctr_on, "\noff", ctr_off, "\nrecords with a second round of phase-2 rows, on / off:", rounds_on, rounds_off)
    assert ctr_off["p2_exact"] == 0 and ctr_off["p2_exact_misses"] == 0 and ctr_on["p2_exact_misses"] == 0, (ctr_on, ctr_off)
    assert rounds_on <= rounds_off, (rounds_on, rounds_off)
    # nothing but phase 2 differs: the tile phase took the same paths
    assert {k: v for k, v in ctr_on.items() if not k.startswith("p2_")} == {k: v for k, v in ctr_off.items() if not k.startswith("p2_")}, (ctr_on, ctr_off)
    return ctr_on, ctr_off, chunks


MACHINE = {
    "defaults": {},
    "block32": {"WFM_TILE_T": "32"},
    "halo_tiles": {"WFM_TILE_THREADS": "256"},
    "narrow_rings": {"WFM_MEM_BUDGET_MB": "256"},
    "chunk1": {"WFM_TILE_CHUNK": "1"},
    "no_reuse": {"WFM_REUSE": "0"},
}


@pytest.mark.parametrize("cfg", sorted(MACHINE))
def test_exact_walk_equals_the_search(monkeypatch, capfd, cfg):
    on, off, chunks = _both(monkeypatch, capfd, MACHINE[cfg], "all", again=cfg == "defaults")
    below = _set("all")[3]
    assert below >= 100
    assert on["p2_exact"] >= below and on["planned_ends"] >= on["p2_exact"], (on, below)
    # below the roots' level a chunk holds nothing but exact jobs: no maxima were taken for it
    assert any(x == 100.0 for _, x in chunks) and any(x == 0.0 for _, x in chunks), chunks


def test_long_gaps_hit_late(monkeypatch, capfd):
    """the roots of tests/reuse_touch_cases.py: their children meet inside inserts of thousands of bases, I2 / D2, the hit at i = u - o2"""
    on, off, _ = _both(monkeypatch, capfd, {}, "touch")
    # (with parent reuse a child whose planned end lies in the block right behind its keep searches, planned_meet_eligible: every planned end is exact)
    assert on["p2_exact"] == on["planned_ends"] > 100, on


def test_byte_kernel_jobs_keep_searching(monkeypatch, capfd):
    on, off, _ = _both(monkeypatch, capfd, {}, "n")
    assert on["p2_exact"] == 0 and on["jobs"] > 2 and on == off, (on, off)


def test_search_jobs_and_exact_jobs_share_a_chunk(monkeypatch, capfd):
    """the N twins next to ordinary pairs: below the roots the twins' jobs search, the others' are exact, in one chunk of phase 2"""
    on, off, chunks = _both(monkeypatch, capfd, {}, "mixed")
    assert on["p2_exact"] >= _set("mixed")[3] > 0, (on, _set("mixed")[3])
    assert any(0.0 < x < 100.0 for _, x in chunks), chunks


def test_a_miss_goes_through_the_search(monkeypatch, capfd):
    """WFM_P2_EXACT_REACH = 1: the walk gives up after the test at the planned end itself; the jobs that hit there keep their answer, the others
    leave with a miss and take the search over the same rows, once -- every record as before, in a chunk that holds search jobs of its own"""
    for name in ("all", "mixed"):
        full, ctr_full, _, _ = _run(monkeypatch, capfd, {}, name)
        short, ctr, _, _ = _run(monkeypatch, capfd, {"WFM_P2_EXACT_REACH": "1"}, name)
        print(name, ctr)
        assert short == full
        assert ctr["p2_exact"] == ctr_full["p2_exact"] and ctr_full["p2_exact_misses"] == 0, (ctr, ctr_full)
        assert 0 < ctr["p2_exact_misses"] < ctr["p2_exact"], ctr
