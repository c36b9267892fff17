"""GPU tests: the BiWFA tile phase at its block boundaries, against the oracle.

run_tiled_phase (wfa_host.hip), wfa_tile_advance_kernel (wfa_kernels.hip) and the two instantiations of wfa_tile2_kernel
(wfa_tile2.hip) are a small state machine: coarse blocks whose meeting block runs again with per-score maxima (mode 5), a third ring
with the block before a short run up to the meeting point run again for its gap rows (mode 6), a workgroup size per block, and the
run up to the meeting point itself (modes 1 -> 2).  Which branch a job takes depends on where its directions meet relative to a
block of T scores.  tests/tile_path_cases.py builds pairs that meet AT those places -- the first step of a block (with a reverse run
of zero steps), around the 26 rows phase 2 reads behind a run, the last step, in blocks 0 .. 3 -- by the oracle's own word
(pyoracle.meet_point), and this file runs them under every switch of the machine.

Per record: status 0, the oracle's score, and ops byte-identical to oracle.align_biwfa -- no tolerance, this path is bit-exact by
contract.  Per configuration: the counters of wfm_get_tile_counters must show that the path it aims at ran.  What must have happened
is derived from the oracle's meeting points of the ROOTS alone (children only add to the counts); a configuration whose counters
say the path did not run fails.
"""
import functools

import pytest

import tile_path_cases as TC
from wfmash_amd import capi

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _set(name):
    """-> (items, oracle ops, oracle scores, [(b, tf, tr)] of the roots, penalties): computed once, shared, never changed"""
    from oracle import pyoracle as O
    pen = TC.ALT_PEN if name == "alt" else None
    T = 32 if name.startswith("t32") else 100
    if name == "wide":
        items = [(p, t) for p, t, _ in TC.wide_set()]
        meet = [TC.classify(sf, sf, T) for _, _, sf in TC.wide_set()]
    else:
        cases = TC.select(T, pen)
        items = [TC.n_twin(c) if name.endswith("n") else (c.p, c.t) for c in cases]
        meet = [TC.classify(c.sf, c.sr, T) for c in cases]
    ops, scores, _, failed = O.align_batch_biwfa([p for p, _ in items], [t for _, t in items], pen)
    assert failed == 0
    return items, ops, [int(s) for s in scores], meet, pen


def _run(monkeypatch, env, name):
    """one align call on a fresh handle under `env` -> (the call's tile counters, its problem flags); every record checked"""
    for k in ("WFM_TILE", "WFM_TILE_T", "WFM_TILE_THREADS", "WFM_TILE_COARSE", "WFM_TILE_COARSE_MIN_BLOCKS", "WFM_TILE_COARSE_MAX_JOBS",
              "WFM_TILE_RING3", "WFM_TILE_FINE", "WFM_TILE_CHUNK", "WFM_TILE_EXACT", "WFM_TILE_FINE_MARGIN", "WFM_P2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    items, ops, scores, meet, pen = _set(name)
    h = capi.Handle(0)
    try:
        res = h.align(items, pen)  # (no hints: the roots have no bound)
        ctr, flags = h.tile_counters(), h.problem_flags(len(items))
    finally:
        h.close()
    bad = [(i, meet[i], r.status, r.score, scores[i]) for i, r in enumerate(res) if r.status != 0 or r.score != scores[i] or r.ops != ops[i]]
    assert not bad, (env, name, bad[:8], len(bad))
    return ctr, flags


def _expect(name):
    meet = _set(name)[3]
    return len(meet), sum(1 for b, tf, tr in meet if b >= 1 and min(tf, tr) < 26)


def _check_machine(ctr, name, packed=True):
    """coarse blocks, third rings and exact ends all on: what the roots alone must have caused"""
    roots, short_runs = _expect(name)
    assert ctr["jobs"] >= roots and ctr["exact_ends"] >= roots, ctr
    assert ctr["left_band"] == 0, ctr
    if packed:
        assert ctr["fine_reruns"] >= roots, ctr      # every root finds its meeting block with one maximum per block, then runs it again
        assert ctr["gap_reruns"] >= short_runs > 0, (ctr, short_runs)
        assert ctr["ring3"] > 0 and ctr["blocks_coarse"] > 0 and ctr["blocks_fine"] > 0, ctr


def _check_twins(ctr, flags, name):
    """the byte kernel's jobs: never a third ring, never a block without per-score maxima of their own making"""
    roots, _ = _expect(name)
    assert ctr["jobs"] >= roots, ctr
    assert ctr["ring3"] == 0 and ctr["gap_reruns"] == 0 and ctr["fine_reruns"] == 0, ctr
    assert len(flags) == roots and all(int(f) & capi.WFM_PF_BYTE_KERNEL for f in flags), flags


MACHINE = {  # configurations that leave every part of the machine on
    "defaults": {},
    "children_coarse": {"WFM_TILE_COARSE_MIN_BLOCKS": "0"},
    "chunk1": {"WFM_TILE_CHUNK": "1"},
    "chunk4_children_coarse": {"WFM_TILE_CHUNK": "4", "WFM_TILE_COARSE_MIN_BLOCKS": "0"},  # mode 5 set inside a host chunk: the job waits for the next
    "uniform_workgroups": {"WFM_TILE_FINE": "0"},
    "no_fine_margin": {"WFM_TILE_FINE_MARGIN": "0", "WFM_TILE_COARSE_MIN_BLOCKS": "0"},    # children's fine_s right at half their score
}


@pytest.mark.parametrize("cfg", sorted(MACHINE))
def test_block_boundaries_whole_machine(monkeypatch, cfg):
    ctr, _ = _run(monkeypatch, MACHINE[cfg], "t100")
    _check_machine(ctr, "t100")
    ctr, flags = _run(monkeypatch, MACHINE[cfg], "t100n")
    _check_twins(ctr, flags, "t100n")
    assert ctr["exact_ends"] >= _expect("t100n")[0], ctr


@pytest.mark.parametrize("extra", [{}, {"WFM_TILE_COARSE_MIN_BLOCKS": "0"}])
def test_block_boundaries_smallest_block(monkeypatch, extra):
    """T = 32 = RING, the smallest block the host allows: the run up to the meeting point is shorter than the rows streamed"""
    env = dict({"WFM_TILE_T": "32", "WFM_TILE_THREADS": "256"}, **extra)
    ctr, _ = _run(monkeypatch, env, "t32")
    _check_machine(ctr, "t32")
    ctr, flags = _run(monkeypatch, env, "t32n")
    _check_twins(ctr, flags, "t32n")


def test_block_boundaries_without_coarse_blocks(monkeypatch):
    ctr, _ = _run(monkeypatch, {"WFM_TILE_COARSE": "0"}, "t100")
    roots, short_runs = _expect("t100")
    assert ctr["fine_reruns"] == 0 and ctr["blocks_coarse"] == 0 and ctr["blocks_fine"] > 0, ctr
    assert ctr["exact_ends"] >= roots and ctr["gap_reruns"] >= short_runs and ctr["ring3"] > 0, ctr
    ctr, flags = _run(monkeypatch, {"WFM_TILE_COARSE": "0"}, "t100n")
    _check_twins(ctr, flags, "t100n")


@pytest.mark.parametrize("extra", [{}, {"WFM_TILE_COARSE_MIN_BLOCKS": "0"}])
def test_block_boundaries_without_third_ring(monkeypatch, extra):
    env = dict({"WFM_TILE_RING3": "0"}, **extra)
    ctr, _ = _run(monkeypatch, env, "t100")
    roots, _ = _expect("t100")
    assert ctr["gap_reruns"] == 0 and ctr["ring3"] == 0, ctr
    assert ctr["exact_ends"] >= roots and ctr["fine_reruns"] >= roots and ctr["blocks_coarse"] > 0, ctr
    ctr, flags = _run(monkeypatch, env, "t100n")
    _check_twins(ctr, flags, "t100n")


def test_both_forms_of_a_switch_in_one_process(monkeypatch):
    """WFM_TILE_RING3 (like WFM_TILE_FINE and WFM_P2) is read per call: a process that has run one form runs the other"""
    a, _ = _run(monkeypatch, {}, "t100")
    b, _ = _run(monkeypatch, {"WFM_TILE_RING3": "0"}, "t100")
    c, _ = _run(monkeypatch, {}, "t100")
    assert a["ring3"] > 0 and b["ring3"] == 0 and c == a, (a, b, c)
    _run(monkeypatch, {"WFM_P2": "0"}, "t100")  # the step kernel takes phase 2 from the exact ends


def test_block_boundaries_chunk_filled_to_zero(monkeypatch):
    """WFM_TILE_COARSE_MAX_JOBS=1: every chunk of more than one job keeps per-score maxima from the first block on"""
    ctr, _ = _run(monkeypatch, {"WFM_TILE_COARSE_MAX_JOBS": "1"}, "t100")
    roots, short_runs = _expect("t100")
    assert ctr["fine_reruns"] == 0 and ctr["blocks_coarse"] == 0, ctr
    assert ctr["exact_ends"] >= roots and ctr["gap_reruns"] >= short_runs, ctr


def test_block_boundaries_inexact_end(monkeypatch):
    """WFM_TILE_EXACT=0: the tile phase stops at the start of the meeting block, the step kernel redoes the block"""
    ctr, _ = _run(monkeypatch, {"WFM_TILE_EXACT": "0"}, "t100")
    assert ctr["jobs"] >= _expect("t100")[0], ctr
    assert ctr["exact_ends"] == 0 and ctr["fine_reruns"] == 0 and ctr["gap_reruns"] == 0 and ctr["ring3"] == 0, ctr
    _run(monkeypatch, {"WFM_TILE_EXACT": "0"}, "t100n")


def test_step_kernel_alone(monkeypatch):
    """WFM_TILE=0: a second device implementation of the same search"""
    ctr, _ = _run(monkeypatch, {"WFM_TILE": "0"}, "t100")
    assert ctr["jobs"] == 0 and ctr["blocks_coarse"] == 0 and ctr["blocks_fine"] == 0, ctr
    ctr, _ = _run(monkeypatch, {"WFM_TILE": "0"}, "t32n")
    assert ctr["jobs"] == 0, ctr


def test_block_boundaries_other_penalties(monkeypatch):
    """penalties (4, 6, 2, 12, 1), the selection made with the oracle at those penalties: the LDS tile kernel, whose end is not exact"""
    ctr, _ = _run(monkeypatch, {}, "alt")
    assert ctr["jobs"] >= _expect("alt")[0], ctr
    assert ctr["exact_ends"] == 0 and ctr["ring3"] == 0 and ctr["blocks_coarse"] == 0 and ctr["blocks_fine"] == 0, ctr


def test_halo_paths(monkeypatch):
    """WFM_TILE_THREADS=256: deep jobs go from one tile without a halo to several tiles with halos on the way, and some jobs meet in the
    first block of several tiles"""
    for extra in ({}, {"WFM_TILE_COARSE_MIN_BLOCKS": "0"}):
        ctr, _ = _run(monkeypatch, dict({"WFM_TILE_THREADS": "256"}, **extra), "wide")
        roots = _expect("wide")[0]
        assert ctr["jobs"] >= roots and ctr["exact_ends"] >= roots and ctr["left_band"] == 0, ctr
