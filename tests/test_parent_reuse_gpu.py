"""GPU tests: a BiWFA child's outer direction from the rows its parent kept (parent reuse: wfa_plan.h, run_tiled_phase and its stages
in wfa_host.hip, wfa_keep_kernel / wfa_restore_kernel in wfa_kernels.hip), against the oracle.

A root keeps a compact copy of its snapshot every WFM_REUSE_EVERY blocks; its first child's forward direction and its second child's
reverse direction start where the root's started, so each child runs its inner direction alone up to the score of the keep it was
handed, takes the kept rows for the other one and goes on as any tiled job -- unless a kept cell touches the child's box, in which
case it gives the keep up and runs from score 0.  Per record: status 0, the oracle's score, ops byte-identical to
oracle.align_biwfa, under WFM_REUSE=1 with WFM_REUSE_EVERY 1, 2 and 4 and under WFM_REUSE=0 -- no tolerance, the path is bit-exact by
contract.  Per configuration the counters of wfm_get_tile_counters and the cells the tile kernels computed.

How many jobs must resume is worked out from the oracle's scores: a breakpoint splits a root's score S into its children's, so one
child has at least S / 2; it resumes from the newest keep at or below floor_T(score / 2 - 48) - T (48: WFM_TILE_FINE_MARGIN), and the
root, whose directions meet near S / 2, kept every multiple of cadence x T below that from 8 T on (WFM_REUSE_MIN_BLOCKS).  So every
root with S / 4 >= 48 + (cadence + 10) T has a child that resumes, the cadence being WFM_REUSE_EVERY rounded up to whole chunks of two
blocks.  The pairs are chosen deep enough for that to hold for every one of them under EVERY = 1, 2 and 4 (T = 32, cadence 4:
S >= 1984; the shallowest pair has 2139), so each configuration must show one resume per root at least.
"""
import functools

import pytest

from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

ENV_KEYS = ("WFM_REUSE", "WFM_REUSE_EVERY", "WFM_REUSE_MIN_BLOCKS", "WFM_SUB_SLACK", "WFM_REUSE_TOUCH_SLACK", "WFM_REUSE_LEVELS", "WFM_TILE", "WFM_TILE_T", "WFM_TILE_CHUNK", "WFM_TILE_THREADS",
            "WFM_TILE_RING3", "WFM_TILE_COARSE", "WFM_TILE_FINE_MARGIN", "WFM_TILE_EXACT")


def _with_n(seq: bytes, at: int) -> bytes:
    return seq[:at] + b"N" + seq[at + 1:]


@functools.lru_cache(maxsize=None)
def _set(name):
    """-> (items, oracle ops, oracle scores): computed once, shared, never changed"""
    from oracle import pyoracle as O
    items = []
    if name == "t32":
        # a dozen pairs of 3 - 8 kb at 5 - 10 % (the shorter the pair, the higher its rate: every root deep enough to hand a keep on);
        # the indels of the mutation process leave the lengths unequal, two pairs are cut to be clearly so, one carries an N
        shapes = [(3300, 0.10), (3500, 0.10), (4000, 0.09), (4500, 0.08), (5000, 0.08), (5500, 0.07), (6000, 0.07), (6500, 0.06),
                  (7000, 0.06), (7500, 0.05), (8000, 0.05), (8000, 0.10)]
        for i, (n, rate) in enumerate(shapes):
            t = synth.random_dna(0x9E05 + i, n)
            q = synth.mutate(t, rate, 0x9E050000 + i)
            if i == 3:
                t = t[:-180]
            if i == 6:
                q = q[:-230]
            if i == 9:
                q = _with_n(q, len(q) // 3)
            items.append((t, q))
    elif name == "t100":
        for i in range(4):  # four pairs of 12 kb at 10 %
            t = synth.random_dna(0x9E15 + i, 12000)
            q = synth.mutate(t, 0.10, 0x9E150000 + i)
            items.append((t[:-150], q) if i == 1 else (t, q))
    elif name == "periodic":
        # microsatellite-like: a unit of 31 bases over and over, a substitution every few dozen bases in both sequences -- the diagonals a period away
        # match as well as the main one
        for i, (n, every) in enumerate([(4030, 37), (5022, 29), (6014, 43)]):
            unit = synth.random_dna(0x9E25 + i, 31)
            base = (unit * (n // 31 + 1))[:n]
            t = synth.mutate(base, 1.0 / every, 0x9E250000 + i, p_sub=1.0, p_ins=0.0)
            q = synth.mutate(base, 1.0 / every, 0x9E260000 + i, p_sub=1.0, p_ins=0.0)
            items.append((t, q))
    else:
        raise ValueError(name)
    ops, scores, _, failed = O.align_batch_biwfa([p for p, _ in items], [t for _, t in items])
    assert failed == 0
    return items, ops, [int(s) for s in scores]


def _run(monkeypatch, env, name):
    """one align call on a fresh handle under `env` -> (tile counters, cells_tile, [(status, score, ops)]); every record checked against the oracle"""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    items, ops, scores = _set(name)
    h = capi.Handle(0)
    try:
        res = h.align(items)
        ctr, cells = h.tile_counters(), int(h.stats().cells_tile)
    finally:
        h.close()
    bad = [(i, r.status, r.score, scores[i]) for i, r in enumerate(res) if r.status != 0 or r.score != scores[i] or r.ops != ops[i]]
    assert not bad, (env, name, bad[:8], len(bad))
    return ctr, cells, [(r.status, r.score, r.ops) for r in res]


def _must_resume(name, T, every, chunk=2):
    cadence = -(-every // chunk) * chunk
    return sum(1 for s in _set(name)[2] if s // 4 >= 48 + (cadence + 10) * T)


def _check_settings(monkeypatch, name, T, base_env):
    off_ctr, off_cells, off_res = _run(monkeypatch, dict(base_env, WFM_REUSE="0"), name)
    print(name, "reuse off:", off_ctr, "cells_tile", off_cells)
    assert off_ctr["reuse_resumed"] == 0 and off_ctr["reuse_fallbacks"] == 0 and off_ctr["reuse_keeps"] == 0, off_ctr
    roots = len(_set(name)[0])
    for every in (1, 2, 4):
        ctr, cells, res = _run(monkeypatch, dict(base_env, WFM_REUSE="1", WFM_REUSE_EVERY=str(every)), name)
        print(name, "reuse every", every, ":", ctr, "cells_tile", cells, "must resume", _must_resume(name, T, every))
        assert res == off_res
        assert ctr["reuse_keeps"] >= 2 * roots, ctr                       # both directions of every root, once at least
        assert _must_resume(name, T, every) == roots                      # the pairs were chosen for it
        assert ctr["reuse_resumed"] >= roots, (ctr, roots)                # one per root
        assert cells < off_cells, (cells, off_cells)


def test_children_resume_small_blocks(monkeypatch):
    """T = 32: the roots are dozens of blocks deep, their children resume after a handful"""
    assert _must_resume("t32", 32, 1) == _must_resume("t32", 32, 2) == _must_resume("t32", 32, 4) == len(_set("t32")[0])
    _check_settings(monkeypatch, "t32", 32, {"WFM_TILE_T": "32"})


def test_children_resume_default_blocks(monkeypatch):
    assert _must_resume("t100", 100, 4) == len(_set("t100")[0])
    _check_settings(monkeypatch, "t100", 100, {})


def test_a_touching_keep_falls_back(monkeypatch):
    """Pairs built on a short period.  Their off-diagonals a period away match to the end of the box, but reaching one costs a gap of a
    period (24 + 31 points and more), so such a diagonal runs behind the main one by that much: it reaches the child's wall when the
    main diagonal is about to end, near the child's full score, while a keep is taken below HALF that score -- no kept cell of these
    pairs touches.  The natural run therefore only has to stay oracle-identical (its fallbacks are printed), and the path is forced
    with WFM_REUSE_TOUCH_SLACK set beyond every offset: every job that takes its keep must then give it up and run from score 0, none
    may be left out, none may differ."""
    for name in ("periodic", "t32"):
        natural = _run(monkeypatch, {"WFM_TILE_T": "32"}, name)
        print(name, "natural:", natural[0])
        forced = _run(monkeypatch, {"WFM_TILE_T": "32", "WFM_REUSE_TOUCH_SLACK": str(1 << 28)}, name)
        print(name, "forced:", forced[0])
        assert forced[2] == natural[2]
        assert forced[0]["reuse_resumed"] == 0, forced[0]
        assert forced[0]["reuse_fallbacks"] >= 1 and forced[0]["reuse_fallbacks"] >= natural[0]["reuse_resumed"], (forced[0], natural[0])


def test_deeper_levels_keep_too(monkeypatch):
    """WFM_REUSE_LEVELS: a child that took its outer direction from its parent keeps the inner one, which it computed from score 0 itself, for the
    one child of its own that starts there; the same records, more jobs resumed than with the roots' keeps alone"""
    for name, env in (("t100", {}), ("t32", {"WFM_TILE_T": "32"})):
        roots_only = _run(monkeypatch, dict(env, WFM_REUSE_LEVELS="1"), name)
        deeper = _run(monkeypatch, dict(env, WFM_REUSE_LEVELS="8"), name)
        print(name, "levels 1:", roots_only[0], roots_only[1], "levels 8:", deeper[0], deeper[1])
        assert deeper[2] == roots_only[2]
        assert deeper[0]["reuse_resumed"] > roots_only[0]["reuse_resumed"], (deeper[0], roots_only[0])
        assert deeper[1] < roots_only[1]
