#!/usr/bin/env python3
"""A/B of two builds of libwfmash_hip.so on a fixed battery of align calls: the results and the integer counters of
build B must be those of build A.  Made for changes of the BiWFA level driver (wfa_host.hip) that must not change a decision.

    python scripts/driver_ab.py --lib-a OLD/libwfmash_hip.so --lib-b wfmash_amd/libwfmash_hip.so --out DIR

Every run is a fresh child process with WFM_LIB_PATH set (capi.py loads that library), under a time limit of its own; a child
starts only if the one before it exited 0.  Build A runs twice first: an integer field that differs between those two runs is
unstable by itself, is listed, and is left out of the comparison -- status, score and ops may not be among them.  Then B runs,
and what is left of its dump has to equal A's byte for byte.  No millisecond field is dumped.

The battery (small shapes, a few seconds):
  a  64 pairs of 0 - 3 kbp, some empty, some unrelated, default budget: three parts on streams of their own
  b  three balanced pairs of 80 kbp at 4 % under 128 MB: guessed bands, grown rings, resumed snapshots
  c  80 kbp against 82 kbp with a score hint of 3000 under 128 MB: the guess fails, the job starts again on a grown band
  d  sixteen pairs of 5 kbp under penalties (5, 8, 2, 100, 1): scope 102, rings of 128 rows, no tiles
  e  sixteen ends-free patch problems
  f  the pairs of a through the run-length entry point
  g  twelve pairs of tests/tile_path_cases (4000 bases) with their N twins in one call, at WFM_TILE_T 100 (g) and 32 (g32): tiles of
     the packed kernel and of the byte kernel in one task list
  h  four pairs of 3 kbp at 15 - 25 % whose phase 2 takes further rounds (more launches of phase 2 than levels)
  i  four ends-free patches of tests/test_align_gpu.py's wide set: base jobs on tiles (wfa_base2t_kernel)
A case of g, h, i that does not show its path in build A's dump ends the run: it is to be replaced, not kept.
"""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUTPUT_FIELDS = ("problems.status", "problems.score", "problems.ops")


def _pairs(seed, n, lens, rates):
    from wfmash_amd import synth
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = rng.choice(lens)
        p = synth.random_dna(seed * 1000 + i, L)
        t = synth.mutate(p, rng.choice(rates), seed * 7919 + i) if L else b""
        r = rng.random()
        if r < 0.08:
            t = synth.random_dna(seed * 31 + i, rng.randrange(0, 400))
        elif r < 0.12:
            t = b""
        elif r < 0.16:
            p = b""
        out.append((p, t))
    return out


def _balanced(seed, length, rate, n):
    from wfmash_amd import synth
    out = []
    while len(out) < n:
        p = synth.random_dna(seed, length)
        t = synth.mutate(p, rate, seed + 0x10000)
        seed += 1
        if abs(len(t) - len(p)) < 64:
            out.append((p, t))
    return out


# (seed, length, mutation rate) of the pairs of case h
H_PAIRS = ((0x3BBA, 3000, 0.17), (0x3BBC, 3000, 0.19), (0x3BBE, 3000, 0.21), (0x3BC0, 3000, 0.23))


def _diverged(seed, length, rate):
    from wfmash_amd import synth
    p = synth.random_dna(seed, length)
    return p, synth.mutate(p, rate, seed + 0x20000)


def _tile_pairs():
    """twelve members of the tile-path family, each followed by its twin with one N"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tile_path_cases as tp
    out = []
    for K, dels, side in [(10, (0, 0, 0, 0), 0), (13, (1, 0, 0, 2), 1), (20, (0, 2, 2, 0), 0), (41, (0, 0, 0, 0), 0), (42, (3, 0, 0, 1), 1), (50, (4, 1, 0, 4), 0),
                          (64, (2, 0, 0, 0), 1), (77, (0, 0, 0, 3), 0), (90, (1, 3, 3, 1), 1), (120, (0, 0, 0, 0), 0), (141, (2, 0, 0, 2), 0), (158, (4, 0, 0, 0), 1)]:
        p, t = tp.make_pair(K, dels, side)
        out += [(p, t), tp.n_twin(tp.Case(K, dels, side, p, t, 0, 0, 0))]
    return out


def _wide_patches():
    """the head and the tail form of the first two shapes of test_wide_patches_on_tiles_match_oracle"""
    from wfmash_amd import capi, synth
    out = []
    for i, (L, div, pre) in enumerate([(3400, 0.10, 0), (3000, 0.14, 0)]):
        p = synth.random_dna(5100 + i, L)
        t = synth.random_dna(5200 + i, pre) + synth.mutate(p, div, 5300 + i)
        out += [(p, t, capi.WFM_MODE_ENDSFREE, len(p), 0, len(t), 0), (p, t, capi.WFM_MODE_ENDSFREE, 0, len(p), 0, len(t))]
    return out


def shows_its_path(dump):
    """-> the cases of g, h, i whose path the dump does not show"""
    from wfmash_amd import capi
    flags = lambda case: [p["flags"] for p in dump[case]["problems"]]
    bad = []
    for g in ("g", "g32"):
        byte = [bool(f & capi.WFM_PF_BYTE_KERNEL) for f in flags(g)]
        if not (any(byte) and not all(byte) and dump[g]["tile"]["jobs"] > 0):
            bad.append(g)
    if not dump["h"]["stats"]["p2_launches"] > dump["h"]["stats"]["levels"]:
        bad.append("h")
    if not all(f & capi.WFM_PF_BASE_TILES for f in flags("i")):
        bad.append("i")
    return bad


def battery():
    """(name, WFM_MEM_BUDGET_MB or None, penalties or None, run-length?, items, further switches of the environment)"""
    from wfmash_amd import capi, synth
    small = _pairs(5, 64, [0, 100, 700, 1500, 3000], [0.0, 0.01, 0.05, 0.15])
    hinted = []
    for i in range(2):
        p = synth.random_dna(0x2001 + i, 80_000)
        t = synth.mutate(p, 0.015, 0x2101 + i)
        t = t[:40_000] + synth.random_dna(0x2201 + i, 2_000 + len(p) - len(t)) + t[40_000:]
        hinted.append((p, t, capi.WFM_MODE_END2END_BIWFA, 0, 0, 0, 0, 3000))
    patches = []
    for p, t in _pairs(9, 16, [300, 600, 1200], [0.02, 0.08]):
        p, t = p or b"ACGT", t or b"ACG"
        patches.append((p, t, capi.WFM_MODE_ENDSFREE, len(p), 0, len(t), 0))
    return [("a", None, None, False, small, {}),
            ("b", 128, None, False, _balanced(0x1001, 80_000, 0.04, 3), {}),
            ("c", 128, None, False, hinted, {}),
            ("d", None, (5, 8, 2, 100, 1), False, _pairs(7, 16, [5000], [0.01, 0.04]), {}),
            ("e", None, None, False, patches, {}),
            ("f", None, None, True, small, {}),
            ("g", None, None, False, _tile_pairs(), {"WFM_TILE_T": "100"}),
            ("g32", None, None, False, _tile_pairs(), {"WFM_TILE_T": "32"}),
            ("h", None, None, False, [_diverged(*spec) for spec in H_PAIRS], {}),
            ("i", None, None, False, _wide_patches(), {})]


def child(dump_path):
    from wfmash_amd import capi
    dump = {"library": capi.LIB_PATH}
    for name, budget_mb, pen, rle, items, env in battery():
        if budget_mb is None:
            os.environ.pop("WFM_MEM_BUDGET_MB", None)
        else:
            os.environ["WFM_MEM_BUDGET_MB"] = str(budget_mb)
        os.environ.update(env)
        h = capi.Handle(0)
        try:
            if rle:
                res = [dict(status=r.status, score=r.score, ops=None if r.ops is None else [[n, op.decode()] for n, op in r.ops], n_runs=r.n_runs,
                            ops_len=ops_len, cells=r.cells) for r, ops_len in h.align_rle(items, pen)]
            else:
                res = [dict(status=r.status, score=r.score, ops=None if r.ops is None else r.ops.decode(), n_runs=r.n_runs, cells=r.cells)
                       for r in h.align(items, pen)]
            for r, f in zip(res, h.problem_flags(len(items))):
                r["flags"] = int(f)
            st = h.stats()
            stats = {k: int(getattr(st, k)) for k, t in capi.Stats._fields_ if not k.startswith("ms_") and k != "pad_"}
            dump[name] = dict(problems=res, stats=stats, tile=h.tile_counters())
        finally:
            h.close()
            for k in env:
                del os.environ[k]
        print(f"case {name}: {len(items)} problems, statuses {sorted(set(r['status'] for r in res))}", flush=True)
    with open(dump_path, "w") as f:
        json.dump(dump, f, sort_keys=True)


def _fields(dump):
    """{(case, field name): value}; a per-problem field's value is the list over the case's problems."""
    out = {}
    for case, d in dump.items():
        if case == "library":
            continue
        for k in d["problems"][0] if d["problems"] else ():
            out[(case, "problems." + k)] = [p[k] for p in d["problems"]]
        for grp in ("stats", "tile"):
            for k, v in d[grp].items():
                out[(case, grp + "." + k)] = v
    return out


def run_child(lib, dump_path, limit):
    env = dict(os.environ, WFM_LIB_PATH=os.path.abspath(lib))
    rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dump_path], env=env, timeout=limit).returncode
    if rc != 0:
        sys.exit(f"the run of {lib} ended with {rc}: nothing more is started")
    return json.load(open(dump_path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="DUMP")
    ap.add_argument("--lib-a")
    ap.add_argument("--lib-b")
    ap.add_argument("--out", default="driver_ab_out")
    ap.add_argument("--limit", type=int, default=240, help="seconds per run")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    os.makedirs(a.out, exist_ok=True)
    first = run_child(a.lib_a, os.path.join(a.out, "a1.json"), a.limit)
    if shows_its_path(first):
        sys.exit("build A does not show the path of: " + ", ".join(shows_its_path(first)))
    a1 = _fields(first)
    a2 = _fields(run_child(a.lib_a, os.path.join(a.out, "a2.json"), a.limit))
    unstable = sorted({k[1] for k in a1 if a1[k] != a2.get(k)})
    print("unstable between two runs of A (left out):", unstable or "none")
    if any(f in OUTPUT_FIELDS for f in unstable):
        sys.exit("an output field differs between two runs of the same library")
    b = _fields(run_child(a.lib_b, os.path.join(a.out, "b.json"), a.limit))
    keep = lambda d: json.dumps({f"{c}:{f}": v for (c, f), v in sorted(d.items()) if f not in unstable}, sort_keys=True)
    ja, jb = keep(a1), keep(b)
    diff = sorted(f"{c}:{f}" for (c, f) in set(a1) | set(b) if f not in unstable and a1.get((c, f)) != b.get((c, f)))
    print(f"compared {len(a1) - sum(1 for k in a1 if k[1] in unstable)} fields of {len({k[0] for k in a1})} cases, {len(ja)} bytes")
    if ja != jb:
        sys.exit("B differs from A in: " + ", ".join(diff))
    print("A/B identical")


if __name__ == "__main__":
    main()
