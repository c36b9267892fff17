"""Pairs for the exact walk of phase 2 beyond those of tests/planned_meet_cases.py (shared by tests/test_p2_exact_cpu.py and
tests/test_p2_exact_gpu.py): short gaps that put a CHILD's breakpoint into I1 / D1, and two long pairs whose rows pass 1024 diagonals."""
import functools

import planned_meet_cases as PM
from wfmash_amd import synth


@functools.lru_cache(maxsize=None)
def short_gap_pairs():
    """-> [(p, t)]: gap_pairs()' construction with ONE gap of 7 or 12 bases in the middle of the FIRST half: the root's directions meet near
    the middle of the pair, and the first child's meet inside the short gap -- a breakpoint in I1 / D1 below the root"""
    out = []
    for i, (K, L, side) in enumerate([(260, 7, 0), (261, 7, 1), (262, 12, 0), (263, 12, 1)]):
        n = 3000
        p = synth.random_dna(0x9AB0 + i, n)
        a = bytearray(p)
        for q in range(K):
            pos = (2 * q + 1) * n // (2 * K)
            a[pos:pos + 1] = a[pos:pos + 1].translate(PM.TC._SUB)
        t = bytes(a)
        mid = n // 4 - 10   # (the root's breakpoint falls a little before the middle: the first child is that much shorter)
        t = t[:mid] + t[mid + L:] if side == 0 else t[:mid] + synth.random_dna(0x9AC0 + i, L) + t[mid:]
        out.append((p, t))
    return out


@functools.lru_cache(maxsize=None)
def long_pairs():
    """-> [(p, t)]: two pairs of 12 kb at 10 %"""
    out = []
    for i in range(2):
        p = synth.random_dna(0x9AD0 + i, 12000)
        out.append((p, synth.mutate(p, 0.10, 0x9AE0 + i)))
    return out
