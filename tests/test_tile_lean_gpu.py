"""GPU tests: the lean snapshot paths of the packed tile kernel (wfa_tile2.hip, WFM_TILE_LEAN) against the oracle and against the general path.

A wave of wfa_tile2_kernel whose diagonals (of the core) lie inside every row it loads (stores) takes 32 (26) unconditional 8-byte accesses in place of a
range test per row; every other wave takes the masked form.  The test that picks the path is wave-uniform and must never change a value, so per
record: status 0, the oracle's score and ops byte-identical to oracle.align_biwfa, and WFM_TILE_LEAN=1 and =0 (read per launch) identical to each
other in one process -- no tolerance, the path is bit-exact by contract.

That both paths ran is derived, not counted on the device: wfmh_test_tile_lean_waves applies the predicate the kernel evaluates
(tile_wave_lean_load / tile_wave_lean_store of wfa_rows.h) to the tiles of a block of a job, and the blocks a root runs follow from the oracle's
meeting point (pyoracle.meet_point) and the plan's geometry (T, threads, core = 2 threads - 2 T).  A root's score bound is not known here (none,
or the greedy bound, which is no smaller than its score): the counts are taken with no bound and with the tightest one possible, the score
itself, and both must show lean waves of both kinds, general waves, and tiles that hold both.

What the counts are and are not.  They model the forward direction of every root with the configured workgroup size in every block; the planner
gives a block whose widest range fits one tile a smaller workgroup (plan_tile_chunk, threads_b), and such a block has no halo and one tile, whose
waves the hook lays out by the range's width whatever `threads` says -- but the counts are those of the model, not of the launches, and only
their being non-zero is asserted.  The short last blocks with wide rows (a lean load under a refused lean store) are the divergent pairs 3 of
"small" (meets at 1424 = 44 x 32 + 16) and 1 of "default" (4513 = 45 x 100 + 13): their seeds were kept because they meet there, which
_check_presence asserts; the tile_path_cases members meet at scores of 33 .. 57, where a row is narrower than a wave and no wave is lean."""
import ctypes as C
import functools

import numpy as np
import pytest

import tile_path_cases as TC
from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

SUB_NONE = 1 << 29
E2E = capi.WFM_MODE_END2END_BIWFA
ENV_KEYS = ("WFM_TILE", "WFM_TILE_T", "WFM_TILE_THREADS", "WFM_TILE_COARSE", "WFM_TILE_COARSE_MIN_BLOCKS", "WFM_TILE_COARSE_MAX_JOBS", "WFM_TILE_RING3",
            "WFM_TILE_FINE", "WFM_TILE_CHUNK", "WFM_TILE_EXACT", "WFM_TILE_FINE_MARGIN", "WFM_P2", "WFM_REUSE", "WFM_TILE_FAST", "WFM_TILE_LEAN")
SMALL = {128: {"WFM_TILE_THREADS": "128", "WFM_TILE_T": "32"}, 256: {"WFM_TILE_THREADS": "256", "WFM_TILE_T": "32"}}


@functools.lru_cache(maxsize=None)
def _set(name):
    """-> (items, oracle ops, oracle scores, [(sf, sr)] of the roots, [the bound a root is known to run under, or None]): computed once, never changed"""
    from oracle import pyoracle as O
    items = []
    if name == "small":
        # divergent pairs whose rows reach a few thousand diagonals: wholly interior tiles, tiles at both ends of a row, one-tile blocks on the way
        for i in range(5):
            n = 1200 + 200 * i
            p = synth.random_dna(0x1EA0 + i, n)
            items.append((p, synth.mutate(p, 0.20 + 0.025 * i, 0x1EA00 + i)))
        # a short last block (Tn < 26: the store test must refuse it), by the oracle's own word: roots that meet early in a block after the first
        short = [c for c in TC.select(32) if TC.classify(c.sf, c.sr, 32)[0] >= 1 and min(TC.classify(c.sf, c.sr, 32)[1:]) < 26]
        assert len(short) >= 3
        items += [(c.p, c.t) for c in short[:4]]
    elif name == "default":
        for i in range(2):
            p = synth.random_dna(0x1EB0 + i, 6000 + 300 * i)
            items.append((p, synth.mutate(p, 0.25, 0x1EB00 + i)))
    else:
        raise KeyError(name)
    ops, scores, _, failed = O.align_batch_biwfa([p for p, _ in items], [t for _, t in items])
    assert failed == 0
    scores = [int(s) for s in scores]
    meet = [O.meet_point(p, t)[:2] for p, t in items]
    subs = [None] * len(items)
    if name == "small":
        # a hinted pair of very unequal lengths whose bound binds: the text is a slice of the pattern, the alignment one long gap; under a bound
        # 700 above the score the rows stop growing at 700-odd diagonals and their upper end moves inwards with every score
        p = synth.random_dna(0x1EC0, 3600)
        t = synth.mutate(p[900:2300], 0.02, 0x1EC00)
        rc, o, sc, _ = O.align_biwfa(p, t)
        assert rc == 0
        items.append((p, t, E2E, 0, 0, 0, 0, sc + 700))
        ops.append(o); scores.append(sc); meet.append(O.meet_point(p, t)[:2]); subs.append(sc + 700)
    return items, ops, scores, meet, subs


@functools.lru_cache(maxsize=None)
def _hook():
    lib = capi.load()
    assert "wfmh_test_tile_lean_waves" in capi.HOST_EXPORTS
    lib.wfmh_test_tile_lean_waves.restype = C.c_int
    lib.wfmh_test_tile_lean_waves.argtypes = [C.c_void_p, C.c_void_p]
    return lib


def _waves(pl, tl, sub, s0, T, Tn, threads):
    """-> (tiles, waves, lean at the load, lean at the store, tiles with both kinds) of one block of one direction"""
    q = np.array([pl, tl, sub, s0, T, Tn, 2 * threads - 2 * T, threads], dtype=np.int32)
    out = np.zeros(5, dtype=np.int64)
    assert _hook().wfmh_test_tile_lean_waves(q.ctypes.data, out.ctypes.data) == 0
    return out


def _expected(name, T, threads, tight):
    """the forward direction of every root, block by block up to its meeting point (the last block takes tf steps)"""
    items, _, scores, meet, subs = _set(name)
    tot = np.zeros(5, dtype=np.int64)
    last_short = np.zeros(5, dtype=np.int64)
    for it, sc, (sf, _), sub in zip(items, scores, meet, subs):
        bound = sub if sub is not None else (sc if tight else SUB_NONE)
        b_meet, tf, _ = TC.classify(sf, sf, T)
        for b in range(b_meet + 1):
            w = _waves(len(it[0]), len(it[1]), bound, b * T, T, tf if b == b_meet else T, threads)
            tot += w
            if b == b_meet and tf < 26:
                last_short += w
    return tot, last_short


def _run(monkeypatch, env, name):
    """the set under `env` with the lean paths on, then off, on fresh handles of one process; every record checked against the oracle and the two forms
    against each other"""
    items, ops, scores, _, _ = _set(name)
    got = []
    for lean in ("1", "0"):
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("WFM_TILE_LEAN", lean)
        h = capi.Handle(0)
        try:
            res = h.align(items)
            ctr = h.tile_counters()
            flags = h.problem_flags(len(items))
        finally:
            h.close()
        bad = [(i, r.status, r.score, scores[i]) for i, r in enumerate(res) if r.status != 0 or r.score != scores[i] or r.ops != ops[i]]
        assert not bad, (env, name, lean, bad[:8], len(bad))
        if env.get("WFM_TILE") != "0":
            assert ctr["jobs"] >= len(items), ctr  # every root went through the tile phase
            assert not any(int(f) & capi.WFM_PF_BYTE_KERNEL for f in flags), flags  # ... on the packed kernel
        got.append([(r.status, r.score, r.ops) for r in res])
    assert got[0] == got[1]


def _check_presence(name, T, threads):
    for tight in (False, True):
        tot, last_short = _expected(name, T, threads, tight)
        tiles, waves, ld, st, mixed = (int(x) for x in tot)
        print(f"{name} T={T} threads={threads} tight={tight}: tiles {tiles} waves {waves} lean load {ld} lean store {st} mixed tiles {mixed}")
        assert ld > 0, tot                        # lean waves at the load
        assert st > 0, tot                        # ... and at the store (a 128-thread tile's two waves both lie partly in the halo: the core's lanes of each)
        assert waves - ld > 0 and waves - st > 0  # and general ones
        assert mixed > 0, tot                     # both kinds in one tile
        assert tiles > 0
        # the short last blocks (wide rows among them, chosen so: lean loads): none of their waves is lean at the store
        assert last_short[1] > 0 and last_short[2] > 0 and last_short[3] == 0, last_short


@pytest.mark.parametrize("threads", [128, 256])
def test_small_tiles_lean_and_general_waves(monkeypatch, threads):
    """tiles of 256 / 512 diagonals with cores of 192 / 448: rows of a few thousand diagonals hold interior tiles, end tiles and one-tile blocks"""
    _check_presence("small", 32, threads)
    _run(monkeypatch, SMALL[threads], "small")


def test_default_tile_size(monkeypatch):
    """two pairs of about 6 kb at 25 %: interior tiles of 1024 diagonals (512 threads, T = 100, cores of 824)"""
    _check_presence("default", 100, 512)
    _run(monkeypatch, {}, "default")


@pytest.mark.parametrize("switch", ["WFM_TILE_COARSE", "WFM_TILE_RING3", "WFM_P2", "WFM_REUSE", "WFM_TILE_FAST"])
def test_lean_paths_under_the_existing_switches(monkeypatch, switch):
    """the small set with one part of the machine off at a time (WFM_TILE_FAST=0: the round-4 form of the kernel shares the prologue and the store)"""
    _run(monkeypatch, dict(SMALL[256], **{switch: "0"}), "small")
