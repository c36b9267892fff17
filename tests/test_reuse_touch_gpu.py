"""GPU tests: parent reuse where a kept wavefront touches the child's box, on real data (wfa_restore_kernel's `touch |= v >= wall`, restore_kept /
reuse_fall_back of wfa_host.hip), against the oracle.

tests/reuse_touch_cases.py builds roots whose breakpoint falls inside or right behind a large indel, so that the gap's ray in the parent's kept rows
runs along the side of a child's box (or a few rows inside it), and classifies every level-1 child from the oracle's rows alone: every keep it can be
handed touches (must touch), none does (must not touch), or it depends.  tests/test_reuse_touch_cases_cpu.py shows that a touching keep is NOT the
child's own rows: a touch the kernel missed -- `>` for `>=`, the wall of the wrong side, the parent's coordinates, the M rows alone -- hands a child
wrong rows.

Each record is a batch of its own on a fresh handle, so the counters of wfm_get_tile_counters are the record's; WFM_REUSE_LEVELS=1: only the root
keeps, only its two children can resume.  Per record, under every configuration: status 0, the oracle's score and ops byte for byte;
reuse_resumed <= 2 - (its must-touch children); no touch counted where both children must not touch; nothing counted at all under WFM_REUSE=0.
Per configuration: the touches counted over the records with a must-touch child are at least half those children, the resumes over the records
whose children both must not touch at least half those children -- the planner decides which scores a root keeps at, so not every child is handed a
keep, but a family the planner sidesteps altogether would prove nothing.
"""
import functools

import pytest

import reuse_touch_cases as R
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

ENV_KEYS = ("WFM_REUSE", "WFM_REUSE_EVERY", "WFM_REUSE_MIN_BLOCKS", "WFM_SUB_SLACK", "WFM_REUSE_TOUCH_SLACK", "WFM_REUSE_LEVELS", "WFM_TILE", "WFM_TILE_T",
            "WFM_TILE_CHUNK", "WFM_TILE_THREADS", "WFM_TILE_RING3", "WFM_TILE_COARSE", "WFM_TILE_FINE_MARGIN", "WFM_TILE_EXACT", "WFM_SCORE_HINT", "WFM_BOUND")
CONFIGS = {
    "t32_every1": (32, {"WFM_TILE_T": "32", "WFM_REUSE_EVERY": "1"}),
    "t32_every2": (32, {"WFM_TILE_T": "32", "WFM_REUSE_EVERY": "2"}),
    "defaults": (100, {}),
    "ring3_off": (100, {"WFM_TILE_RING3": "0"}),
    "reuse_off": (100, {"WFM_REUSE": "0"}),
}
REUSE_COUNTERS = ("reuse_resumed", "reuse_fallbacks", "reuse_keeps", "reuse_touched", "reuse_fell_other")


@functools.lru_cache(maxsize=None)
def _oracle():
    """-> (items, oracle ops, oracle scores): computed once, shared, never changed"""
    from oracle import pyoracle as O
    items = [(r.p, r.t) for r in R.roots()]
    ops, scores, _, failed = O.align_batch_biwfa([p for p, _ in items], [t for _, t in items])
    assert failed == 0
    assert [int(s) for s in scores] == [r.score for r in R.roots()]
    return items, ops, [int(s) for s in scores]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_touching_keeps_fall_back_and_the_others_resume(monkeypatch, name):
    T, env = CONFIGS[name]
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("WFM_REUSE_LEVELS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    items, ops, scores = _oracle()
    rows, bad = [], []
    for ri, item in enumerate(items):
        h = capi.Handle(0)
        try:
            r = h.align([item])[0]
            ctr = h.tile_counters()
        finally:
            h.close()
        if r.status != 0 or r.score != scores[ri] or r.ops != ops[ri]:
            bad.append((ri, r.status, r.score, scores[ri]))
        cls = tuple(R.classify(ri, di, T).name for di in (0, 1))
        rows.append((ri, cls, ctr))
        print(name, "root", ri, R.roots()[ri].spec.kind, "d", R.roots()[ri].spec.d, cls, {k: ctr[k] for k in REUSE_COUNTERS})
    assert not bad, (name, bad[:8], len(bad))
    for ri, cls, ctr in rows:
        assert ctr["reuse_fallbacks"] == ctr["reuse_touched"] + ctr["reuse_fell_other"], (name, ri, ctr)
        if name == "reuse_off":
            assert all(ctr[k] == 0 for k in REUSE_COUNTERS), (name, ri, ctr)
            continue
        assert ctr["reuse_resumed"] <= 2 - cls.count("touch"), (name, ri, cls, ctr)
        if cls == ("clear", "clear"):
            assert ctr["reuse_touched"] == 0, (name, ri, cls, ctr)
    touch_set = [(cls, ctr) for _, cls, ctr in rows if "touch" in cls]
    clear_set = [(cls, ctr) for _, cls, ctr in rows if cls == ("clear", "clear")]
    n_touch, n_clear = sum(cls.count("touch") for cls, _ in touch_set), 2 * len(clear_set)
    total = {k: (sum(c[k] for _, c in touch_set), sum(c[k] for _, c in clear_set), sum(c[k] for _, _, c in rows)) for k in REUSE_COUNTERS}
    print(name, "must-touch children", n_touch, "children of roots that must not touch", n_clear, "(must-touch set, must-not-touch set, all):", total)
    if name == "reuse_off":
        return
    assert n_touch >= 16 and n_clear >= 16
    assert 2 * total["reuse_touched"][0] >= n_touch, (name, total, n_touch)
    assert 2 * total["reuse_resumed"][1] >= n_clear, (name, total, n_clear)

