"""GPU tests of wfm_sketch_intersections (wfmash_amd/csrc/map_isect.hip): every cell of the matrix against a two-pointer merge
written here, on sketch lengths around every wave, workgroup and LDS boundary, on both forms of the kernel, on real pooled
MinHash sketches, and its argument errors."""
import numpy as np
import pytest

from oracle import map_ani as ANI
from oracle import map_pipeline as MP
from wfmash_amd import capi, synth
from tests.test_map_paf_gpu import _pangenome

pytestmark = pytest.mark.gpu

U64_MAX = np.iinfo(np.uint64).max
LENGTHS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 20000)  # wave and workgroup remainders, the LDS limit from both sides, the global form


def _two_pointer(a, b):
    """map_stats.hpp:719-731 as written, in plain Python (small inputs only)."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    i = j = shared = 0
    while i < len(a) and j < len(b):
        if a[i] == b[j]:
            shared += 1; i += 1; j += 1
        elif a[i] < b[j]:
            i += 1
        else:
            j += 1
    return shared


class _Merge:
    """The same count for long sketches: per value the smaller of the two multiplicities, summed (checked against the loop above)."""

    def __init__(self, sketches):
        self.uc = [np.unique(np.asarray(s, dtype=np.uint64), return_counts=True) for s in sketches]

    def __call__(self, i, j):
        (ua, ca), (ub, cb) = self.uc[i], self.uc[j]
        _, ia, ib = np.intersect1d(ua, ub, assume_unique=True, return_indices=True)
        return int(np.minimum(ca[ia], cb[ib]).sum())

    def matrix(self, rows, cols):
        return np.array([[self(i, j) for j in cols] for i in rows], dtype=np.uint32).reshape(len(rows), len(cols))


def _edge_sketches():
    """Seven kinds of content at each of the nine lengths; neighbours in the list overlap by construction."""
    rng = np.random.default_rng(0x15EC7)
    out = []
    for n in LENGTHS:
        dense = np.sort(rng.integers(0, max(4, n), n, dtype=np.uint64))               # random, many duplicates, shares values with every dense sketch
        out.append(dense)
        wide = np.sort(rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2))   # random over the whole range, all even
        out.append(wide)
        out.append(wide.copy())                                                       # an identical pair
        out.append(wide + np.uint64(1) if n else wide.copy())                         # a disjoint pair (all odd)
        out.append(np.full(n, 3, dtype=np.uint64))                                    # one value through the whole sketch (3 occurs in the dense ones)
        tail = dense.copy()
        if n:
            tail[n - (n + 2) // 3:] = tail[-1]                                        # a run of equal values that ends at the last element
        out.append(tail)
        ends = wide.copy()
        if n:
            ends[:(n + 3) // 4] = 0                                                   # the values 0 and 2^64 - 1, each several times
            ends[n - (n + 3) // 4:] = U64_MAX
        out.append(ends)
    return out


@pytest.fixture(scope="module")
def edge():
    sk = _edge_sketches()
    merge = _Merge(sk)
    small = [i for i, s in enumerate(sk) if len(s) <= 65]
    for i in small:  # the numpy form is the loop
        for j in small:
            assert merge(i, j) == _two_pointer(sk[i], sk[j]), (i, j)
    return sk, merge


def _subsets(n, n_rows, n_cols, seed):
    rng = np.random.default_rng(seed)
    rows, cols = rng.permutation(n)[:n_rows], rng.permutation(n)[:n_cols]
    assert n_rows + n_cols <= n or len(set(rows.tolist()) & set(cols.tolist())) > 0
    return rows.astype(np.int32), cols.astype(np.int32)


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (37, 41)])
def test_edge_lengths_every_cell_is_the_two_pointer_count(gpu, edge, shape):
    sk, merge = edge
    assert len(sk) == 63
    for seed in (1, 2) if shape != (37, 41) else (3,):
        rows, cols = _subsets(len(sk), shape[0], shape[1], seed * 100 + shape[1])
        if shape == (1, 1):  # the single cell: the longest sketch against itself shifted, then the repeated value against a dense one
            rows, cols = (np.array([8 * 7 + 1], dtype=np.int32), np.array([8 * 7 + 2], dtype=np.int32)) if seed == 1 else \
                (np.array([7 * 7 + 4], dtype=np.int32), np.array([8 * 7], dtype=np.int32))
        got = gpu.sketch_intersections(sk, rows, cols)
        assert got.dtype == np.uint32 and got.shape == shape
        exp = merge.matrix(rows, cols)
        assert (got == exp).all(), np.argwhere(got != exp)[:5]
    if shape == (37, 41):
        assert len(set(rows.tolist()) & set(cols.tolist())) > 10 and set(rows.tolist()) != set(cols.tolist())
        assert exp.max() >= 4097  # a long sketch met itself, its twin or its like


def test_every_kind_against_every_kind_at_every_length(gpu, edge):
    """all 63 x 63 cells: one value on one side and on both, runs that end a sketch, 0 and 2^64-1, empty against everything"""
    sk, merge = edge
    got = gpu.sketch_intersections(sk)
    exp = merge.matrix(range(len(sk)), range(len(sk)))
    assert (got == exp).all(), np.argwhere(got != exp)[:5]
    assert (got == got.T).all()
    assert (np.diag(got) == [len(s) for s in sk]).all()
    assert (got[:7] == 0).all()                                        # the empty sketches
    full3 = [7 * k + 4 for k in range(len(LENGTHS))]                   # one value through the whole sketch, on both sides: the shorter length
    assert got[full3[8], full3[7]] == 4097 and got[full3[5], full3[8]] == 4095
    assert got[7 * 6 + 6, 7 * 8 + 6] == 2 * ((4096 + 3) // 4)          # zeros and 2^64-1 of the 4096 sketch inside those of the 20000 one


def test_matrix_in_many_launches_is_the_same_matrix(gpu, edge, monkeypatch):
    """WFM_ISECT_CELLS bounds a launch: 100 cells make row blocks of two whole rows, 7 cells cut every row into pieces of columns"""
    sk, merge = edge
    rows, cols = _subsets(len(sk), 37, 41, 77)
    exp = merge.matrix(rows, cols)
    for cells in ("100", "7", "1"):
        monkeypatch.setenv("WFM_ISECT_CELLS", cells)
        got = gpu.sketch_intersections(sk, rows, cols)
        assert (got == exp).all(), cells


def test_both_forms_agree(gpu):
    """a column of WFM_ISECT_LDS_MAX hashes is searched in LDS; the same contents with one more, largest, hash in global memory"""
    assert capi.ISECT_LDS_MAX == 4096
    rng = np.random.default_rng(4097)
    col = np.sort(rng.integers(0, 3000, 4096, dtype=np.uint64))       # duplicates: ranks inside runs matter
    col_long = np.concatenate([col, np.array([U64_MAX], dtype=np.uint64)])
    others = [np.sort(rng.integers(0, 3000, n, dtype=np.uint64)) for n in (1, 65, 4096, 9000)]
    others.append(np.concatenate([others[2][:4000], np.full(96, U64_MAX, dtype=np.uint64)]))   # holds the extra hash, 96 times
    sk = [col, col_long] + others
    merge = _Merge(sk)
    got = gpu.sketch_intersections(sk, rows=np.arange(len(sk)), cols=[0, 1])
    exp = merge.matrix(range(len(sk)), [0, 1])
    assert (got == exp).all(), (got, exp)
    assert merge(2, 0) == _two_pointer(sk[2], col) and merge(3, 1) == _two_pointer(sk[3], col_long)
    same = [0, 2, 3, 4, 5]
    assert (got[same, 0] == got[same, 1]).all()      # the extra hash is shared with nobody but ...
    assert got[6, 1] == got[6, 0] + 1                # ... the sketch that holds it 96 times, once
    assert got[0, 1] == 4096 and got[1, 1] == 4097


def test_real_pooled_sketches_all_vs_all(gpu):
    seqs = _pangenome(51)
    names = [n for n, _ in seqs] + ["repeat#1#r"]
    bases = [s for _, s in seqs] + [synth.random_dna(5, 300) * 150]   # 4096 hashes, fewer than 400 distinct values
    groups = MP.ref_groups(names)
    pooled = {}
    for g, sq in zip(groups, bases):
        pooled[g] = ANI.pool(pooled.get(g, np.zeros(0, dtype=np.uint64)), gpu.minhash_sketch(sq))
    sk = [pooled[g] for g in sorted(pooled)]
    assert len(sk) == 9 and max(len(s) for s in sk) == 4096 and min(len(s) for s in sk) < 1000
    rep = sk[sorted(pooled).index(groups[-1])]
    assert len(rep) == 4096 and len(set(rep.tolist())) < 400
    got = gpu.sketch_intersections(sk)
    merge = _Merge(sk)
    exp = merge.matrix(range(len(sk)), range(len(sk)))
    assert merge(0, 1) == _two_pointer(sk[0], sk[1])
    assert (got == exp).all(), (got, exp)
    assert (got == got.T).all() and (np.diag(got) == [len(s) for s in sk]).all()
    assert got[0, 1] > 1000                                            # two haplotypes of one backbone share most of a sketch


def test_argument_errors_leave_the_handle_usable(gpu):
    rng = np.random.default_rng(9)
    good = [np.sort(rng.integers(0, 500, n, dtype=np.uint64)) for n in (100, 300, 200, 50)]
    exp = _Merge(good).matrix(range(4), range(4))

    def still_works():
        assert (gpu.sketch_intersections(good) == exp).all()

    still_works()
    bad = [s.copy() for s in good]
    bad[2][100] = bad[2][101] + 1                                     # one descending pair inside sketch 2 of 4
    assert (np.diff(bad[2].astype(np.int64)) < 0).sum() == 1
    with pytest.raises(capi.WfmError, match="sketch 2 is not ascending"):
        gpu.sketch_intersections(bad)
    still_works()
    # the last hash of one sketch above the first of the next is no descent
    assert good[0][-1] > good[1][0]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in good])]).astype(np.int64)
    o = offs.copy(); o[0] = 1
    with pytest.raises(capi.WfmError, match=r"offsets\[0\]"):
        gpu.sketch_intersections(good, offsets=o)
    still_works()
    o = offs.copy(); o[2] = o[1] - 1
    with pytest.raises(capi.WfmError, match="decrease"):
        gpu.sketch_intersections(good, offsets=o)
    still_works()
    with pytest.raises(capi.WfmError, match=r"cols\[1\] = 4"):
        gpu.sketch_intersections(good, rows=[0, 1], cols=[3, 4])
    still_works()
    with pytest.raises(capi.WfmError, match=r"rows\[0\] = -1"):
        gpu.sketch_intersections(good, rows=[-1], cols=[0])
    still_works()
    # nothing to compute is no error
    assert gpu.sketch_intersections(good, rows=[], cols=[0, 1]).shape == (0, 2)
    assert gpu.sketch_intersections(good, rows=[0], cols=[]).shape == (1, 0)
