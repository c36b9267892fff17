"""CPU test of the case builder of the tile-path tests (tests/tile_path_cases.py): coverage is a condition, not a hope.  Every class
of meeting point the GPU test (tests/test_tile_paths_gpu.py) is about must be IN the selections, by the oracle's own word."""
import pytest

import tile_path_cases as TC


@pytest.mark.parametrize("T,pen", [(100, None), (32, None), (100, TC.ALT_PEN)])
def test_selection_holds_every_required_class(oracle, T, pen):
    cases = TC.select(T, pen)
    have = TC.covered(cases, T)
    missing = [c for c in TC.required(T, pen) if c not in have]
    assert not missing, missing
    # what is in the selection is the oracle's answer for the pair as built, not the model's guess
    for c in cases[::7]:
        assert (c.p, c.t) == TC.make_pair(c.K, c.dels, c.side)
        assert oracle.meet_point(c.p, c.t, pen) == (c.sf, c.sr, c.last_fwd)
    if pen is None:
        assert 80 <= len(cases) <= 120, len(cases)
        # the list of the issue, spelled out: every edge in every block of 1 .. 3, (1, 0) and (T, T) among them
        for b in (1, 2, 3):
            for e in [(1, 0), (1, 1), (2, 1), (25, 24), (25, 25), (26, 25), (26, 26), (27, 26), (27, 27),
                      (T - 1, T - 2), (T - 1, T - 1), (T, T - 1), (T, T)]:
                assert (b,) + e in have
        assert {(0, T, T), (0, T, T - 1), (0, 25, 25), (0, 25, 24)} <= have  # block 0: no block before it to run again
        assert any(c[0] >= 1 and min(c[1], c[2]) < 26 for c in have) and any(c[0] >= 1 and min(c[1], c[2]) >= 26 for c in have)
    # both shapes: the deletions taken from the text (tl < pl) and from the pattern (tl > pl), and pairs without any
    assert sum(len(c.t) < len(c.p) for c in cases) >= 8 and sum(len(c.t) > len(c.p) for c in cases) >= 8
    assert sum(len(c.t) == len(c.p) for c in cases) >= 2
    assert all(len(c.p) <= TC.N and len(c.t) <= TC.N for c in cases)
    assert all(0 < c.sf <= 4 * T for c in cases)


def test_n_twins_meet_where_their_pairs_do(oracle):
    """one N at the same place of pattern and text matches itself: same meeting point, same score -- on the byte kernels"""
    for T in (100, 32):
        for c in TC.select(T)[::8]:
            p, t = TC.n_twin(c)
            assert p.count(b"N") == 1 and t.count(b"N") == 1 and len(p) == len(c.p) and len(t) == len(c.t)
            assert oracle.meet_point(p, t) == (c.sf, c.sr, c.last_fwd)
            assert oracle.align_biwfa(p, t)[2] == oracle.align_biwfa(c.p, c.t)[2]


def test_wide_set_reaches_the_first_block_of_several_tiles(oracle):
    """WFM_TILE_THREADS=256, T = 100: a tile holds 512 diagonals, the host's range of the block that ends at score s is 2 s + 1 wide, and
    a chunk is two blocks -- blocks 0 and 1 are one tile without a halo, the block of scores 201 .. 300 is the first of several"""
    ws = TC.wide_set()
    deep = [w for w in ws if 1500 <= len(w[0]) <= 3000]
    assert len(deep) == 16 and all(w[2] > 300 for w in deep)  # they cross from the one form to the other on the way
    first = [w for w in ws if 200 < w[2] <= 300]
    assert len(first) >= 4
    assert all(min(len(p), 300) + min(len(t), 300) + 1 > 512 - 2 * 100 for p, t, _ in first)  # wider than one core there: halos
