"""The deal of a target subset's sequences over the handles of wfmh_map_multi (wfmh_test_deal; no GPU): longest first onto the
least-loaded handle, ties to the lower index -- the rule of wfmash_amd/dist.py:shard_records."""
import ctypes as C

from wfmash_amd import capi
from wfmash_amd.dist import shard_records

LENGTHS = [((i * 7919) % 97 + 1) * 1000 + (i % 3) for i in range(61)] + [50_000] * 5  # (with ties)


def _loads(lengths, part, n_parts):
    loads = [0] * n_parts
    for ln, p in zip(lengths, part):
        loads[p] += ln
    return loads


def test_every_index_is_assigned_exactly_once():
    for n_parts in (1, 2, 3, 8):
        part = capi.host_deal(LENGTHS, n_parts)
        assert len(part) == len(LENGTHS)
        assert all(0 <= p < n_parts for p in part)
        assert set(part) == set(range(n_parts))


def test_two_calls_give_the_same_answer():
    assert capi.host_deal(LENGTHS, 8) == capi.host_deal(LENGTHS, 8)
    assert capi.host_deal(list(LENGTHS), 3) == capi.host_deal(tuple(LENGTHS), 3)


def test_no_load_exceeds_the_lightest_by_more_than_the_longest_item():
    for n_parts in (2, 3, 4, 8):
        loads = _loads(LENGTHS, capi.host_deal(LENGTHS, n_parts), n_parts)
        assert max(loads) - min(loads) <= max(LENGTHS), (n_parts, loads)


def test_fewer_items_than_parts_leaves_the_surplus_parts_empty():
    # longest first, each onto an empty part, ties to the lower index: the parts beyond the items stay empty
    assert capi.host_deal([5, 9, 7], 8) == [2, 0, 1]
    assert capi.host_deal([4, 4], 3) == [0, 1]
    assert capi.host_deal([], 4) == []


def test_the_rule_is_that_of_shard_records():
    for n_parts in (1, 3, 8):
        part = capi.host_deal(LENGTHS, n_parts)
        shards = shard_records(LENGTHS, n_parts)
        assert [sorted(i for i, p in enumerate(part) if p == g) for g in range(n_parts)] == shards


def test_bad_arguments_are_refused():
    L = capi.load()
    L.wfmh_test_deal.restype = C.c_int
    L.wfmh_test_deal.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    out = (C.c_int32 * 2)()
    ln = (C.c_int64 * 2)(3, 4)
    assert L.wfmh_test_deal(ln, 2, 0, out) != 0
    assert L.wfmh_test_deal(None, 2, 2, out) != 0
