#!/usr/bin/env python3
"""A/B of two builds of libwfmash_hip.so on a fixed battery of align calls: the output file and the integer fields of the summary
of build B must be those of build A.  Made for changes of the align phase's host side (host/aligner.cpp, host/wflign_hip.cpp,
host/cigar_ops.hpp) that must not change a byte.

    python scripts/align_driver_ab.py --lib-a OLD/libwfmash_hip.so --lib-b wfmash_amd/libwfmash_hip.so --out DIR

Every run is a fresh child process with WFM_LIB_PATH set (capi.py loads that library), under a time limit of its own; a child
starts only if the one before it exited 0, and one child runs at a time (it holds at most two handles).  A library runs once per
setting of the environment, because the driver reads its switches once per process.  Build A runs twice first: a field that differs
between those two runs is unstable by itself, is listed, and is left out of the comparison -- only the summary's times (ms_*) may
be among them.  Then B runs, and what is left of its dump has to equal A's.

The battery, on the input of tests/test_align_paf_gpu.py (five haplotypes of 40 kb, 24 chains of one to three pieces, a row that
does not parse):
  paf            the defaults
  sam_md         SAM with the MD tag
  sam_noseq      SAM without SEQ
  nopatch        disable_chain_patching, no padding
  resident       resident_sequences, PAF (lazy fetches)
  resident_sam   resident_sequences, SAM with MD
  short          the rows of 100 - 280, 300 - 800 and 4000 bases, no padding: the late-tail call
  two_handles    wfmh_align_paf_multi with two handles on the one GPU
Under a switch of the environment -- WFM_ALIGN_WORKERS=1 and =3, WFM_ALIGN_MIN_BATCHES=4 and =8 (several batches: the caps on
records and bases are not parameters of the C ABI), WFM_ALIGN_OWN_HANDLES=0 -- paf, resident and short; and once paf with
WFM_RECORD_TAGS, whose file is compared sorted by row number (batches write it as they finish).
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

SETTINGS = ("", "WFM_ALIGN_WORKERS=1", "WFM_ALIGN_WORKERS=3", "WFM_ALIGN_MIN_BATCHES=4", "WFM_ALIGN_MIN_BATCHES=8", "WFM_ALIGN_OWN_HANDLES=0",
            "WFM_RECORD_TAGS=tags.tsv")
UNDER_A_SWITCH = ("paf", "resident", "short")

BATTERY = [("paf", {}, 1),
           ("sam_md", {"sam_format": 1, "emit_md_tag": 1}, 1),
           ("sam_noseq", {"sam_format": 1, "no_seq_in_sam": 1}, 1),
           ("nopatch", {"disable_chain_patching": 1, "target_padding": 0, "query_padding": 0}, 1),
           ("resident", {"resident_sequences": 1}, 1),
           ("resident_sam", {"resident_sequences": 1, "sam_format": 1, "emit_md_tag": 1}, 1),
           ("short", {"target_padding": 0, "query_padding": 0}, 1),
           ("two_handles", {}, 2)]


def short_rows(seqs, names):
    rng = random.Random(5)
    qn, tn = names[0], names[2]
    lines = []
    for k in range(36):
        seg = (rng.randrange(100, 280), rng.randrange(300, 800), 4000)[k % 3]
        qs = rng.randrange(200, 30000 - seg)
        lines.append("\t".join(map(str, [qn, len(seqs[qn]), qs, qs + seg, "+", tn, len(seqs[tn]), qs + rng.randrange(-20, 20),
                                         qs + seg + rng.randrange(-20, 20), 100, seg, 30, "id:f:0.95", "kc:f:0.9", f"ch:Z:{k + 1}.1.1"])))
    return lines


def child(dump_path, workdir, only):
    import pathlib
    from tests.test_align_paf_gpu import _make_case
    from wfmash_amd import capi
    fa, paf, seqs, _ = _make_case(pathlib.Path(workdir), 21)
    short = os.path.join(workdir, "short.paf")
    with open(short, "w") as f:
        f.write("\n".join(short_rows(seqs, list(seqs))) + "\n")
    tags = os.environ.get("WFM_RECORD_TAGS")
    dump = {"library": capi.load()._name}
    handles = [capi.Handle(0), capi.Handle(0)]
    try:
        for name, over, nh in BATTERY:
            if only and name not in only:
                continue
            out = os.path.join(workdir, name + ".out")
            if tags and os.path.exists(tags):
                os.remove(tags)
            P = dict(over, threads=16)
            rows = short if name == "short" else paf
            s = capi.align_paf(handles[0], fa, rows, out, params=P) if nh == 1 else capi.align_paf_multi(handles[:nh], fa, rows, out, params=P)
            d = {"text": open(out).read()}
            for k, _ in capi.AlignSummary._fields_:
                d["summary." + k] = getattr(s, k)
            if tags:
                d["tags_sorted"] = sorted(open(tags).read().splitlines(), key=lambda l: int(l.split("\t")[0]))
            dump[name] = d
            print(f"case {name}: {s.written} of {s.records} records written, {s.batches} batches", flush=True)
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
        env = dict(os.environ, WFM_LIB_PATH=os.path.abspath(lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", dump_path, "--workdir", workdir]
        if setting:
            k, v = setting.split("=")
            env[k] = os.path.join(os.path.abspath(workdir), v) if k == "WFM_RECORD_TAGS" else v
            cmd += ["--only", "paf" if k == "WFM_RECORD_TAGS" else ",".join(UNDER_A_SWITCH)]
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env).returncode
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
    ap.add_argument("--out", default="align_driver_ab_out")
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.workdir, set(a.only.split(",")) if a.only else None)
    os.makedirs(a.out, exist_ok=True)
    a1 = run_children(a.lib_a, "a1", a.out, a.limit)
    if not all(a1[k] for k in a1 if k[2] == "summary.written"):
        sys.exit("build A: a case wrote no record")
    if a1[("WFM_ALIGN_MIN_BATCHES=4", "paf", "summary.batches")] < 2:
        sys.exit("build A: WFM_ALIGN_MIN_BATCHES=4 gave one batch")
    a2 = run_children(a.lib_a, "a2", a.out, a.limit)
    unstable = sorted({k[2] for k in a1 if a1[k] != a2.get(k)})
    print("unstable between two runs of A (left out):", unstable or "none")
    if any(not f.startswith("summary.ms_") for f in unstable):
        sys.exit("a field that is no time differs between two runs of the same library")
    b = run_children(a.lib_b, "b", a.out, a.limit)
    diff = sorted(f"{s or 'defaults'}:{c}:{f}" for (s, c, f) in set(a1) | set(b) if f not in unstable and a1.get((s, c, f)) != b.get((s, c, f)))
    kept = [k for k in a1 if k[2] not in unstable]
    print(f"compared {len(kept)} fields of {len({k[:2] for k in a1})} runs, {sum(len(a1[k]) for k in kept if k[2] == 'text')} bytes of output")
    if diff:
        sys.exit("B differs from A in: " + ", ".join(diff))
    print("A/B identical")


if __name__ == "__main__":
    main()
