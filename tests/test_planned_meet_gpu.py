"""The planned end of phase 1 on the GPU (WFM_TILE_PLANNED_END; TileJob::plan_sum, wfa_tile_advance_kernel's tile_plan_enter): jobs whose
score is known go to the run up to a planned state instead of searching for their meeting point, and every record must come out as before.

Pairs of about 4000 bases from tests/planned_meet_cases.py, picked with the oracle so that a child's planned end falls at tf in {1, 25, 26, 27,
T - 1, T} of three consecutive blocks -- the blocks 1 to 3 at T = 100 (from tf = 26 of block 1 on) and 3 to 5 at T = 32: a job that stays with
the breakpoint search has a score above 250, so its planned end lies at sf >= 126 and never in an earlier block -- plus the pairs whose root
meets inside a long gap (children that end or begin in a gap component).  WFM_TILE_T = 128 puts planned ends into the FIRST block (the host's
set-up).  They run through wfm_align_batch under the configurations of MACHINE with WFM_TILE_PLANNED_END = 1 and = 0 in one process: status,
score and op string of every record equal oracle.align_biwfa's and the other form's.  That the path ran is read from wfm_get_tile_counters:
planned ends >= the jobs below the roots in the oracle's recursion (all of them are eligible: packed, bounded, tiled), none with the switch off
or for pairs with an N (the byte kernel).  A call always contains its roots, so "a batch of children only" is a LEVEL of the call below the
first: the WFM_DEBUG line of every tile phase gives its level, its launches of either instantiation of the packed kernel and its mode-5 and
mode-6 reruns (they add up to the call's counters, which is asserted).  Below level 1 no job takes a mode-5 rerun, none a mode-6 rerun
unless WFM_TILE_PLANNED_DEEP = 0 asks for them, and where the chunks launch both instantiations none of their blocks launches the one with
per-score maxima; what is left is level 1's, at most one rerun of either kind a root, the same with the switch off (_children_alone).
Record tags: no more records whose overlap walk needed a second round of rows than with the switch off.
"""
import collections
import functools
import re

import pytest

import planned_meet_cases as PM
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

ENV_KEYS = ("WFM_TILE", "WFM_TILE_T", "WFM_TILE_THREADS", "WFM_TILE_COARSE", "WFM_TILE_COARSE_MIN_BLOCKS", "WFM_TILE_COARSE_MAX_JOBS", "WFM_TILE_RING3",
            "WFM_TILE_FINE", "WFM_TILE_CHUNK", "WFM_TILE_EXACT", "WFM_TILE_FINE_MARGIN", "WFM_P2", "WFM_REUSE", "WFM_REUSE_EVERY", "WFM_REUSE_MIN_BLOCKS",
            "WFM_TILE_PLANNED_END", "WFM_TILE_PLANNED_DEEP", "WFM_SUB_SLACK")


def _n_twin(p, t):
    """the pair with one N at the same place of both sequences, where they agree and the eight bases around agree too: the byte kernels"""
    pos = next(q for q in range(150, 400) if p[q - 8:q + 8] == t[q - 8:q + 8])
    return p[:pos] + b"N" + p[pos + 1:], t[:pos] + b"N" + t[pos + 1:]


@functools.lru_cache(maxsize=None)
def _set(name):
    """-> (items, oracle ops, oracle scores, jobs below the roots in the oracle's recursion): computed once, shared, never changed"""
    from oracle import pyoracle as O
    if name == "n":
        items = [_n_twin(*PM.select(100)[q]) for q in (0, 5)]
    else:
        items = list(PM.select(32 if name == "t32" else 100)) + list(PM.gap_pairs())
    ops, scores, _, failed = O.align_batch_biwfa([p for p, _ in items], [t for _, t in items], None)
    assert failed == 0
    below = sum(len(PM.descendants(p, t)) for p, t in items)
    return items, ops, [int(s) for s in scores], below


LEVEL_LINE = re.compile(r"level (\d+): tiled (\d+) jobs, (\d+) blocks of .* without / with per-score maxima (\d+) / (\d+), mode-5 reruns (\d+), mode-6 reruns (\d+)")
Level = collections.namedtuple("Level", "level jobs blocks coarse fine reruns5 reruns6")  # one tile phase of a level, from its WFM_DEBUG line
Both = collections.namedtuple("Both", "on off lv_on lv_off err")


def _run(monkeypatch, capfd, env, name):
    """one align call on a fresh handle under `env` -> (records, tile counters, problem flags, the tile phases' debug lines, stderr); every
    record checked against the oracle"""
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
    levels = [Level(*(int(x) for x in m)) for m in LEVEL_LINE.findall(err)]
    # the lines add up to the call's counters: nothing the assertions below read level by level is missing from them
    assert (sum(l.coarse for l in levels), sum(l.fine for l in levels)) == (ctr["blocks_coarse"], ctr["blocks_fine"]), (levels, ctr)
    assert (sum(l.reruns5 for l in levels), sum(l.reruns6 for l in levels)) == (ctr["fine_reruns"], ctr["gap_reruns"]), (levels, ctr)
    return [(r.status, r.score, r.ops) for r in res], ctr, [int(f) for f in flags], levels, err


def _both(monkeypatch, capfd, env, name):
    """the switch on, off and on again in one process -> Both: counters and per-level lines of the first two, the stderr of all three"""
    on, ctr_on, fl_on, lv_on, e1 = _run(monkeypatch, capfd, dict(env, WFM_TILE_PLANNED_END="1"), name)
    off, ctr_off, fl_off, lv_off, e2 = _run(monkeypatch, capfd, dict(env, WFM_TILE_PLANNED_END="0"), name)
    again, ctr_again, _, _, e3 = _run(monkeypatch, capfd, env, name)  # (the default is on; read per call, not frozen by the process's first)
    assert on == off == again
    assert ctr_off["planned_ends"] == 0, ctr_off
    assert ctr_again == ctr_on, (ctr_on, ctr_again)
    rounds = [sum(1 for f in fl if f & capi.WFM_PF_P2_ROUNDS) for fl in (fl_on, fl_off)]
    print("records with a second round of phase-2 rows, on / off:", rounds)
    assert rounds[0] <= rounds[1], rounds
    print("on ", ctr_on, lv_on)
    print("off", ctr_off, lv_off)
    return Both(ctr_on, ctr_off, lv_on, lv_off, e1 + e2 + e3)


def _children_alone(b, name, two_forms, deep=True):
    """The levels below the roots' are batches of children only (level 1 is the roots': a call always contains them, and nothing but the
    roots of these sets runs there).  With the switch on none of their jobs takes a mode-5 rerun, none a mode-6 rerun where the gap rows are
    written at once (`deep`, the default), and where the chunks launch both instantiations (`two_forms`: the coarse path is open to the
    children) none of their blocks launches the one with per-score maxima -- so every rerun and every such launch of the call is level 1's,
    at most one rerun of either kind a root."""
    n = len(_set(name)[0])
    on = b.on
    first = [l for l in b.lv_on if l.level == 1]
    below = [l for l in b.lv_on if l.level > 1]
    assert first and below and sum(l.jobs for l in first) == n, (n, b.lv_on)
    assert sum(l.jobs for l in below) == on["planned_ends"] == on["jobs"] - n, (on, b.lv_on)   # every job below the roots took its planned end
    assert all(l.reruns5 == 0 for l in below), below
    assert on["fine_reruns"] == sum(l.reruns5 for l in first) <= n, (on, first)
    if deep:
        assert all(l.reruns6 == 0 for l in below), below
        assert on["gap_reruns"] == sum(l.reruns6 for l in first) <= n, (on, first)
    if two_forms:
        assert all(l.fine == 0 and l.coarse == l.blocks for l in below), below
        assert on["blocks_fine"] == sum(l.fine for l in first), (on, first)
        # with the switch off the children's last blocks needed the instantiation with per-score maxima; the roots' level is the same in both
        # (its parts finish in any order)
        assert sum(l.fine for l in b.lv_off if l.level > 1) > 0, b.lv_off
        assert sorted(l[1:] for l in b.lv_off if l.level == 1) == sorted(l[1:] for l in first), (b.lv_on, b.lv_off)
    else:
        assert all(l.coarse + l.fine == l.blocks for l in below), below   # one launch a block, whichever instantiation the chunk keeps


MACHINE = {
    "defaults": {},
    "children_coarse": {"WFM_TILE_COARSE_MIN_BLOCKS": "0"},
    "no_third_ring": {"WFM_TILE_RING3": "0"},
    "chunk1": {"WFM_TILE_CHUNK": "1"},
    "chunk4": {"WFM_TILE_CHUNK": "4", "WFM_TILE_COARSE_MIN_BLOCKS": "0"},
    "halo_tiles": {"WFM_TILE_THREADS": "256"},
    "all_fine": {"WFM_TILE_COARSE": "0"},
    "step_kernel_phase2": {"WFM_P2": "0"},     # wfa_bp_kernel takes phase 2 from the planned end: its first loop must not go on from there
    "first_block": {"WFM_TILE_T": "128"},      # sf of 126 .. 128 lies in block 0: the host enters the run at set-up
    "rerun_for_gap_rows": {"WFM_TILE_PLANNED_DEEP": "0"},  # the block before a short run up to the planned end runs again (mode 6) instead of writing its 26 gap rows at once
}
TWO_FORMS = ("children_coarse", "chunk4")  # WFM_TILE_COARSE_MIN_BLOCKS = 0: chunks as shallow as these launch the instantiation without per-score maxima


@pytest.mark.parametrize("cfg", sorted(MACHINE))
def test_planned_ends_at_block_edges(monkeypatch, capfd, cfg):
    b = _both(monkeypatch, capfd, MACHINE[cfg], "t100")
    on, off = b.on, b.off
    below = _set("t100")[3]
    assert below >= 48
    assert on["planned_ends"] >= below and on["exact_ends"] >= on["planned_ends"] and on["left_band"] == 0, (on, below)
    assert on["exact_ends"] == off["exact_ends"] and on["jobs"] == off["jobs"], (on, off)
    _children_alone(b, "t100", cfg in TWO_FORMS, deep=cfg != "rerun_for_gap_rows")
    if cfg == "rerun_for_gap_rows":
        # planned ends at tf = 1 and 25 of blocks with a block before them: that block runs again for its gap rows (mode 6), as the block before
        # a meeting point that was searched for does (tf = 1 and 25 of three blocks; the planned end is not the trigger: the count may differ
        # from the search's)
        assert sum(l.reruns6 for l in b.lv_on if l.level > 1) >= 6, b.lv_on
    if cfg == "all_fine":
        assert on["blocks_coarse"] == 0, on


@pytest.mark.parametrize("extra", [{}, {"WFM_TILE_COARSE_MIN_BLOCKS": "0"}])
def test_planned_ends_smallest_block(monkeypatch, capfd, extra):
    b = _both(monkeypatch, capfd, dict({"WFM_TILE_T": "32", "WFM_TILE_THREADS": "256"}, **extra), "t32")
    below = _set("t32")[3]
    assert b.on["planned_ends"] >= below > 0 and b.on["left_band"] == 0, (b.on, below)
    _children_alone(b, "t32", bool(extra))


@functools.lru_cache(maxsize=None)
def _behind_a_restore(name, T, margin):
    """The planner's own answers (wfa_plan.h through the CPU hooks) for every job below the roots of a set, for a parent that holds a keep at
    every block boundary (WFM_REUSE_EVERY = 1, WFM_REUSE_MIN_BLOCKS = 1, WFM_TILE_CHUNK = 1): the keep reuse_pick_keep takes, the block
    planned_meet_block puts the planned end in, and planned_meet_eligible's verdict behind that keep
    -> (jobs that resume, those of them whose planned block is the one right behind the keep, jobs that must keep searching)"""
    import ctypes as C
    import numpy as np
    from oracle import pyoracle as O
    lib = capi.load()
    lib.wfmh_test_reuse_plan.restype = lib.wfmh_test_planned_meet.restype = C.c_int
    lib.wfmh_test_reuse_plan.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    lib.wfmh_test_planned_meet.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    resume = edge = search = 0
    for p, t in _set(name)[0]:
        for j in PM.descendants(p, t):
            kept = list(range(T, j.score + 1, T))
            a = np.array([j.score, T, margin, 1] + kept, dtype=np.int64)
            out = np.zeros(2, dtype=np.int64)
            assert lib.wfmh_test_reuse_plan(0, a.ctypes.data, len(kept), out.ctypes.data) == 0
            s_keep = kept[int(out[0])] if out[0] >= 0 else 0
            q = np.array(list(O.DEFAULT_PEN) + [j.score, j.cb, j.ce, j.second, j.score + 56, 1, 1, 0, 1, s_keep, T], dtype=np.int64)
            got = np.zeros(8, dtype=np.int64)
            assert lib.wfmh_test_planned_meet(q.ctypes.data, 1, got.ctypes.data) == 0
            block, ok = int(got[4]), int(got[7])
            assert ok == (s_keep == 0 or block >= s_keep + T)
            resume += s_keep > 0
            edge += s_keep > 0 and block == s_keep + T
            search += not ok
    return resume, edge, search


@pytest.mark.parametrize("margin", [48, 0])
def test_planned_end_behind_a_restore(monkeypatch, capfd, margin):
    """Parent reuse with a keep at every block: a child resumes from the newest of its parent's keeps at or below floor_T(score / 2 - margin) - T.
    With the default margin of 48 the block of every planned end lies behind that keep's block, for many children right behind it (the keep one
    block before the planned end): all of them take the planned end.  With a margin of 0 the planned end of some children (tf = T: score / 2 a
    multiple of T; a cut inside a gap, whose opening the plan subtracts) lies in the block that begins AT the keep, the first one after the
    restore, whose input holds no gap rows 26 deep: planned_meet_eligible refuses those IF they resume there, and they search as before.  Which
    children are which is the planner's answer on the CPU (_behind_a_restore) for a parent that holds every keep; a parent holds fewer (a
    root keeps nothing at its first look, a job that resumed a direction keeps none of that direction below the resume), and a child without
    its keep starts at score 0 and is eligible again.  So the planned ends lie between the jobs the planner can never refuse and all of them,
    and every job below the roots that is not among them searches: only those may run a block again."""
    env = {"WFM_TILE_CHUNK": "1", "WFM_REUSE_EVERY": "1", "WFM_REUSE_MIN_BLOCKS": "1", "WFM_TILE_FINE_MARGIN": str(margin)}
    b = _both(monkeypatch, capfd, env, "t100")
    on, off = b.on, b.off
    below = _set("t100")[3]
    resume, edge, search = _behind_a_restore("t100", 100, margin)
    print("below", below, "resume", resume, "planned block right behind the keep", edge, "must search", search)
    assert resume > 0 and edge > 0 and (search > 0) == (margin == 0), (resume, edge, search)
    assert on["reuse_resumed"] > 0 and off["reuse_resumed"] > 0, (on, off)
    assert on["reuse_fallbacks"] <= off["reuse_fallbacks"], (on, off)
    # a child that did not resume after all (its parent's rows did not hold its own) is eligible again: never fewer planned ends than these
    assert below - search <= on["planned_ends"] <= below, (on, below, search)
    assert on["reuse_resumed"] <= resume, (on, resume)
    # the roots' reruns are level 1's, at most one of either kind a root; below them only a job that searches may run a block again
    n = len(_set("t100")[0])
    first = [l for l in b.lv_on if l.level == 1]
    lower = [l for l in b.lv_on if l.level > 1]
    assert first and lower and sum(l.reruns5 for l in first) <= n and sum(l.reruns6 for l in first) <= n, b.lv_on
    assert all(l.reruns5 == 0 for l in lower) and sum(l.reruns6 for l in lower) <= below - on["planned_ends"], (on, below, b.lv_on)


def test_planned_ends_on_narrow_rings(monkeypatch, capfd):
    """a budget the levels' full rings do not fit: the children run on the narrow rings the level chooses from their known scores (the flagship
    workload's case) -- the planned end and the rows phase 2 reads behind it lie inside such a ring"""
    monkeypatch.setenv("WFM_MEM_BUDGET_MB", "256")
    b = _both(monkeypatch, capfd, {}, "t100")
    narrow = [int(x) for x in re.findall(r"narrow rings: (\d+) jobs", b.err)]
    # (a narrow ring has to halve the full one, which the deeper, shorter jobs' do not: as many narrow rings a call as it has roots is asked for)
    assert len(narrow) == 3 and min(narrow) >= len(_set("t100")[0]), narrow
    assert b.on["planned_ends"] >= _set("t100")[3] and b.on["left_band"] == 0 and b.off["left_band"] == 0, (b.on, b.off)
    _children_alone(b, "t100", False)


def test_byte_kernel_jobs_keep_searching(monkeypatch, capfd):
    b = _both(monkeypatch, capfd, {}, "n")
    assert b.on["planned_ends"] == 0 and b.on["jobs"] > 2 and b.on == b.off and b.lv_on == b.lv_off, (b.on, b.off)


def test_unbounded_children_keep_searching(monkeypatch, capfd):
    """WFM_SUB_SLACK of 2^28: children run without their parents' scores as a bound -- not eligible"""
    b = _both(monkeypatch, capfd, {"WFM_SUB_SLACK": str(1 << 28)}, "t100")
    assert b.on["planned_ends"] == 0, b.on
