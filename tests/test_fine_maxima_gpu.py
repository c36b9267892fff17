"""GPU tests: the per-score maxima of the packed tile kernel's FINE instantiation, kept in LDS slots.

wfa_tile2_kernel<.., false, true, true, MS> (wfa_tile2.hip) keeps a score's maximum antidiagonal in MS words of LDS shared by all waves of the
workgroup -- a lane's slot is lane & (MS - 1), one ds_max_i32 per step -- and reduces the slots once behind the step loop.  MS follows the
workgroup's size (tile_fine_slots, wfa_device.h: 2 for one wave, 4 up to 128 threads, 16 beyond), so every size is its own layout
[T + 1][MS].  What can go wrong is an index: a score's row of slots one off (the meeting points of tests/tile_path_cases.py sit on the first
and last step of a block, where that shows), a slot that some lane's maximum never reaches, a reduction that leaves a slot out.

Per record: status 0, the oracle's score, ops byte-identical to oracle.align_biwfa -- no tolerance.  The references are the ones
tests/test_tile_paths_gpu.py computes (its cached _set), shared and never changed.
"""
import functools
import re

import pytest

from test_tile_paths_gpu import _set
from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

ENV_KEYS = ("WFM_TILE", "WFM_TILE_T", "WFM_TILE_THREADS", "WFM_TILE_COARSE", "WFM_TILE_COARSE_MIN_BLOCKS", "WFM_TILE_COARSE_MAX_JOBS",
            "WFM_TILE_RING3", "WFM_TILE_FINE", "WFM_TILE_CHUNK", "WFM_TILE_EXACT", "WFM_TILE_FINE_MARGIN", "WFM_TILE_FAST", "WFM_TILE_LEAN",
            "WFM_P2", "WFM_DEBUG")


def _align(monkeypatch, env, items, ops, scores, pen=None):
    """one align call on a fresh handle under `env`; every record compared -> the call's tile counters"""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = capi.Handle(0)
    try:
        res = h.align(items, pen)
        ctr = h.tile_counters()
    finally:
        h.close()
    assert len(res) == len(items)
    bad = [(i, r.status, r.score, scores[i]) for i, r in enumerate(res) if r.status != 0 or r.score != scores[i] or r.ops != ops[i]]
    assert not bad, (env, bad[:8], len(bad))
    return ctr


def _ran_with(capfd):
    """the tile widths (diagonals: two per thread of the largest workgroup) the host says it tiled with -- its WFM_DEBUG line per level"""
    return {int(w) for w in re.findall(r"tiled \d+ jobs, \d+ blocks of \d+ scores \(Wt (\d+)\)", capfd.readouterr().err)}


def _threads_for(asked, T):
    """what the host makes of WFM_TILE_THREADS: a tile beside others keeps 2 * threads - 2 T diagonals of its own between its halos, and a size
    that keeps none is raised by whole waves to the first that does (tile_cfg, wfa_host.hip)"""
    while 2 * asked <= 2 * T:
        asked += 64
    return asked


@pytest.mark.parametrize("threads", [64, 128, 256, 512, 1024])
def test_every_block_fine_every_workgroup_size(monkeypatch, capfd, threads):
    """WFM_TILE_COARSE=0: every block of every job keeps per-score maxima.  The workgroups of a block are as small as its widest range allows
    (whole waves, up to WFM_TILE_THREADS), so every size runs the shapes up to its own"""
    items, ops, scores, meet, pen = _set("t100")
    capfd.readouterr()
    ctr = _align(monkeypatch, {"WFM_TILE_COARSE": "0", "WFM_TILE_THREADS": str(threads), "WFM_DEBUG": "1"}, items, ops, scores, pen)
    assert _ran_with(capfd) == {2 * _threads_for(threads, 100)}
    assert ctr["exact_ends"] >= len(meet) and ctr["jobs"] >= len(meet) and ctr["left_band"] == 0, ctr
    assert ctr["blocks_coarse"] == 0 and ctr["fine_reruns"] == 0 and ctr["blocks_fine"] > 0, ctr


def test_every_block_fine_smallest_block(monkeypatch, capfd):
    """T = 32: rows of 33 scores' slots; the first block of a job is one wave wide (the one-wave instantiation and its two slots)"""
    items, ops, scores, meet, pen = _set("t32")
    capfd.readouterr()
    ctr = _align(monkeypatch, {"WFM_TILE_COARSE": "0", "WFM_TILE_T": "32", "WFM_TILE_THREADS": "256", "WFM_DEBUG": "1"}, items, ops, scores, pen)
    assert _ran_with(capfd) == {512}
    assert ctr["exact_ends"] >= len(meet) and ctr["left_band"] == 0, ctr
    assert ctr["blocks_coarse"] == 0 and ctr["blocks_fine"] > 0, ctr


def test_every_block_fine_several_workgroups_a_score(monkeypatch, capfd):
    """the halo paths: a score's maximum comes from several workgroups, each with slots of its own, through the global maximum"""
    items, ops, scores, meet, pen = _set("wide")
    capfd.readouterr()
    ctr = _align(monkeypatch, {"WFM_TILE_COARSE": "0", "WFM_TILE_THREADS": "256", "WFM_DEBUG": "1"}, items, ops, scores, pen)
    assert _ran_with(capfd) == {512}
    assert ctr["jobs"] >= len(meet) and ctr["exact_ends"] >= len(meet) and ctr["left_band"] == 0, ctr
    assert ctr["blocks_coarse"] == 0 and ctr["blocks_fine"] > 0, ctr


SHIFTS = tuple(range(64)) + (64, 127, 128, 129, 200)
APPENDED = 37  # the pair whose text also goes on behind the pattern


@functools.lru_cache(maxsize=None)
def _shifted():
    """-> (items, oracle ops, oracle scores): a 600-base pattern; the text is the pattern with 6 evenly spaced substitutions and d random bases
    in front of it, d over SHIFTS -- the alignment's leading diagonal, and with it the lane and the slot that hold a score's maximum, moves
    by one from pair to pair, across every slot count and across a wave's edge.  Computed once, shared, never changed"""
    from oracle import pyoracle as O
    n = 600
    p = synth.random_dna(0xF15E, n)
    a = bytearray(p)
    for i in range(6):
        pos = (2 * i + 1) * n // 12
        a[pos:pos + 1] = a[pos:pos + 1].translate(bytes.maketrans(b"ACGT", b"CGTA"))
    body = bytes(a)
    lead = synth.random_dna(0xF15F, max(SHIFTS))
    items = [(p, lead[:d] + body + (lead[d:2 * d] if d == APPENDED else b"")) for d in SHIFTS]
    ops, scores, _, failed = O.align_batch_biwfa([p for p, _ in items], [t for _, t in items], None)
    assert failed == 0
    return items, ops, [int(s) for s in scores]


@pytest.mark.parametrize("env", [{}, {"WFM_TILE_COARSE": "0"}], ids=["defaults", "all_fine"])
def test_maximum_in_every_lane_and_slot(monkeypatch, env):
    items, ops, scores = _shifted()
    assert len(items) == 69 and min(scores) >= 30  # (six substitutions at least)
    ctr = _align(monkeypatch, env, items, ops, scores)
    assert ctr["jobs"] > 0 and ctr["blocks_fine"] > 0 and ctr["left_band"] == 0, ctr
