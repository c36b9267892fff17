#!/usr/bin/env python3
"""A/B of two builds of libwfmash_hip.so on a fixed battery of map calls: the mapping PAF, the scaffold file and the integer
fields of the summary of build B must be those of build A.  Made for changes of the map driver (host/mapper.cpp) that must not
change a byte.

    python scripts/map_driver_ab.py --lib-a OLD/libwfmash_hip.so --lib-b wfmash_amd/libwfmash_hip.so --out DIR

Every run is a fresh child process with WFM_LIB set (capi.py loads that library), under a time limit of its own; a child starts
only if the one before it exited 0, and one child runs at a time (it holds at most two handles).  A library runs once per
setting of the environment -- the defaults, WFM_FILTER_OVERLAP=0, WFM_FILTER_WORKERS=1, WFM_FILTER_DEVICE_ORDER=0 -- because a
build may read these once per process.  Build A runs twice first: a field that differs between those two runs is unstable by
itself, is listed, and is left out of the comparison -- only the summary's times (ms_*) may be among them.  Then B runs, and what is
left of its dump has to equal A's.

The battery, on the pangenome of tests/test_map_paf_gpu.py (six haplotypes of 30 kb, one of them reversed, one with a deletion
and soft masking, a sequence shorter than a window and an unrelated one), at 85 % identity:
  defaults      one subset, one batch of all queries
  subsets       index_by_size 45000: four subsets
  filter1/2/3   the filter modes (map, one-to-one, none) over those subsets
  nosplit       split 0 (without the scaffold filter, which keeps nothing of unchained mappings)
  scaffold      --scaffold-out over the subsets; the file is compared as sorted lines (its line order across queries was never fixed)
  two_handles   wfmh_map_multi with two handles on the one GPU, over the subsets
  index_w, index_r   -W writes the index file of the subsets, -I maps from it
Under a switch of the environment: defaults, subsets, scaffold and two_handles.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SETTINGS = ("", "WFM_FILTER_OVERLAP=0", "WFM_FILTER_WORKERS=1", "WFM_FILTER_DEVICE_ORDER=0")
UNDER_A_SWITCH = ("defaults", "subsets", "scaffold", "two_handles")


def battery(workdir):
    """(name, parameter overrides, handles)"""
    idx = os.path.join(workdir, "pan.idx")
    sub = {"index_by_size": 45000}
    return [("defaults", {}, 1),
            ("subsets", sub, 1),
            ("filter1", dict(sub, filter_mode=1), 1),
            ("filter2", dict(sub, filter_mode=2), 1),
            ("filter3", dict(sub, filter_mode=3), 1),
            ("nosplit", {"split": 0, "scaffold_gap": 0}, 1),
            ("scaffold", dict(sub, scaffold_out=os.path.join(workdir, "scaffolds.tsv")), 1),
            ("two_handles", sub, 2),
            ("index_w", dict(sub, index_file=idx, write_index=1), 1),
            ("index_r", dict(index_file=idx, write_index=0), 1)]


def child(dump_path, workdir, only):
    from tests.test_map_paf_gpu import _pangenome, _write_fasta
    from wfmash_amd import capi
    fa = os.path.join(workdir, "pan.fa")
    _write_fasta(fa, _pangenome(41))
    dump = {"library": capi.load()._name}
    handles = [capi.Handle(0), capi.Handle(0)]
    try:
        for name, over, nh in battery(workdir):
            if only and name not in only:
                continue
            P = capi.map_default_params(percentage_identity=0.85, auto_pct_identity=0, threads=8, **over)
            out = os.path.join(workdir, name + ".paf")
            s = capi.map_paf(handles[0], fa, out, params=P) if nh == 1 else capi.map_paf_multi(handles[:nh], fa, out, params=P)
            d = {"paf": open(out).read()}
            for k, _ in capi.MapSummary._fields_:
                if k != "pad_":
                    d["summary." + k] = getattr(s, k)
            if "scaffold_out" in over:
                d["scaffold_sorted"] = sorted(open(over["scaffold_out"]).read().splitlines())
            if name == "index_w":
                d["index_bytes"] = os.path.getsize(over["index_file"])
            dump[name] = d
            print(f"case {name}: {len(d['paf'].splitlines())} records, {s.subsets} subsets, {s.l2_mappings} mappings", flush=True)
    finally:
        for h in handles:
            h.close()
    with open(dump_path, "w") as f:
        json.dump(dump, f, sort_keys=True)


def run_children(lib, tag, outdir, limit):
    """one child per setting of the environment -> {(setting, case, field): value}"""
    fields = {}
    for i, setting in enumerate(SETTINGS):
        workdir = os.path.join(outdir, f"{tag}_{i}")
        os.makedirs(workdir, exist_ok=True)
        dump_path = os.path.join(workdir, "dump.json")
        env = dict(os.environ, WFM_LIB=os.path.abspath(lib))
        if setting:
            k, v = setting.split("=")
            env[k] = v
        cmd = [sys.executable, os.path.abspath(__file__), "--child", dump_path, "--workdir", workdir]
        if setting:
            cmd += ["--only", ",".join(UNDER_A_SWITCH)]
        rc = subprocess.run(cmd, env=env, timeout=limit).returncode
        if rc != 0:
            sys.exit(f"the run of {lib} ({setting or 'defaults'}) ended with {rc}: nothing more is started")
        for case, d in json.load(open(dump_path)).items():
            if case != "library":
                for k, v in d.items():
                    fields[(setting, case, k)] = v
    return fields


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="DUMP")
    ap.add_argument("--workdir")
    ap.add_argument("--only", default="")
    ap.add_argument("--lib-a")
    ap.add_argument("--lib-b")
    ap.add_argument("--out", default="map_driver_ab_out")
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.workdir, set(a.only.split(",")) if a.only else None)
    os.makedirs(a.out, exist_ok=True)
    a1 = run_children(a.lib_a, "a1", a.out, a.limit)
    if not all(a1[k] for k in a1 if k[2] == "paf" and k[1] != "index_w") or a1[("", "subsets", "summary.subsets")] < 2:
        sys.exit("build A: a case wrote no record, or the subsets case has one subset")
    a2 = run_children(a.lib_a, "a2", a.out, a.limit)
    unstable = sorted({k[2] for k in a1 if a1[k] != a2.get(k)})
    print("unstable between two runs of A (left out):", unstable or "none")
    if any(not f.startswith("summary.ms_") for f in unstable):
        sys.exit("a field that is no time differs between two runs of the same library")
    b = run_children(a.lib_b, "b", a.out, a.limit)
    diff = sorted(f"{s or 'defaults'}:{c}:{f}" for (s, c, f) in set(a1) | set(b) if f not in unstable and a1.get((s, c, f)) != b.get((s, c, f)))
    kept = [k for k in a1 if k[2] not in unstable]
    print(f"compared {len(kept)} fields of {len({k[:2] for k in a1})} runs, {sum(len(a1[k]) for k in kept if k[2] == 'paf')} bytes of PAF")
    if diff:
        sys.exit("B differs from A in: " + ", ".join(diff))
    print("A/B identical")


if __name__ == "__main__":
    main()
