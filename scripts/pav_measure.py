"""What --pav costs (profiles/pav.md).  Two parts:

  stage FASTA OUTDIR [REPS] [WINDOW]
                   the command line end to end on FASTA all-vs-all (-p 90 -P 50k -t 16), REPS times without a switch and REPS times with
                   --pav-window WINDOW (1000), alternating, host clock around the child process; then one run of each with WFM_DEBUG=1,
                   of which the lines of pav_records (`[wflign] pav:`), of the call (`[wfm] pav`) and of the finish (`[wfmash::align]
                   pav:`) are printed.  The PAF with the switch is held against the PAF without.
  union N [N ...]  a synthetic list of N random segments of 50 .. 2000 bases over 2^31 target bases and 8 groups, imported into a fresh
                   object: host clock around wfm_pav_union (it ends in a synchronise), the union's size, a second union of the union
                   with as many new segments again, the matrix of 10 000 intervals x 8 groups; with WFM_DEBUG=1, so that the library's
                   own lines name the device blocks the object holds.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfmash_amd import capi  # noqa: E402

CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")


def stage(fa, outdir, reps, window):
    os.makedirs(outdir, exist_ok=True)

    def run(name, pav, debug=False):
        out = os.path.join(outdir, name + ".paf")
        args = [CLI, "-p", "90", "-P", "50k", "-t", "16", "--out", out]
        if pav:
            args += ["--pav-window", str(window), "--pav-out", os.path.join(outdir, name + ".pav")]
        env = dict(os.environ)
        if debug:
            env["WFM_DEBUG"] = "1"
        t0 = time.perf_counter()
        r = subprocess.run(["timeout", "-k", "10", "300"] + args + [fa], capture_output=True, text=True, env=env)
        ms = (time.perf_counter() - t0) * 1e3
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit("the command line failed (%d): stopping" % r.returncode)
        return round(ms, 1), r.stderr

    run("warm_off", False)
    run("warm_pav", True)
    res = {"off": [], "pav": []}
    for _ in range(reps):
        res["off"].append(run("off", False)[0])
        res["pav"].append(run("pav", True)[0])
    same = open(os.path.join(outdir, "off.paf"), "rb").read() == open(os.path.join(outdir, "pav.paf"), "rb").read()
    table = open(os.path.join(outdir, "pav.pav")).read().splitlines()
    print(json.dumps({"process_ms": res, "paf_equal_to_off": same, "records": sum(1 for _ in open(os.path.join(outdir, "off.paf"))),
                      "rows": len(table) - 1, "columns": table[0].split("\t")[5:], "table_bytes": os.path.getsize(os.path.join(outdir, "pav.pav"))}), flush=True)
    _, err = run("debug_pav", True, debug=True)
    for line in err.splitlines():
        if "pav" in line and (line.startswith("[wflign] pav:") or line.startswith("[wfm] pav") or line.startswith("[wfmash::align] pav:") or line.startswith("[wfmash::pav]")):
            print(line, flush=True)
        if line.startswith("[wflign] coverage:") or line.startswith("[wflign] lift:"):
            print(line, flush=True)
    # the device call alone, on the problems of the PAF just written: a process's first call, then fresh objects and a second add
    from tests import pav_model as M
    names, lengths = sequence_table(fa)
    cols = M.columns(names)
    problems = M.problems_of_paf([l.rstrip("\n") for l in open(os.path.join(outdir, "off.paf"))], names, lengths, cols)
    probs, words = [], []
    for base, runs, g in problems:
        probs.append((base, len(words), len(runs), g))
        words += M.words(runs)
    words = np.asarray(words, dtype=np.uint32)
    h = capi.Handle(0)
    ms = []
    for _ in range(reps + 1):
        pav = h.pav(sum(lengths), len(cols))
        t0 = time.perf_counter()
        pav.add(probs, words)
        t1 = time.perf_counter()
        pav.add(probs, words)
        t2 = time.perf_counter()
        pav.union()
        t3 = time.perf_counter()
        ms.append([round((t1 - t0) * 1e3, 3), round((t2 - t1) * 1e3, 3), round((t3 - t2) * 1e3, 3)])
        pav.close()
    h.close()
    print(json.dumps({"wfm_pav_add through capi (building the numpy problems included)": {"problems": len(probs), "runs": len(words),
                      "[first add of a fresh object, second add, union] ms, the first row the process's first": ms}}), flush=True)


def sequence_table(fasta):
    """names and lengths in file order"""
    import gzip
    names, lengths = [], []
    with (gzip.open(fasta, "rt") if fasta.endswith(".gz") else open(fasta)) as f:
        for line in f:
            if line.startswith(">"):
                names.append(line[1:].split()[0])
                lengths.append(0)
            else:
                lengths[-1] += len(line.strip())
    return names, lengths


def union(sizes):
    h = capi.Handle(0)
    os.environ["WFM_DEBUG"] = "1"  # the library's own `[wfm] pav union` lines name the device blocks the object holds
    n_bases, n_groups = 1 << 31, 8
    rng = np.random.default_rng(7)
    iv = [(int(a), int(a) + 100000) for a in rng.integers(0, n_bases - 100000, 10000)]
    for n in sizes:
        def segs():
            s = np.zeros(n, dtype=capi.PAV_SEG_DTYPE)
            s["length"] = rng.integers(50, 2000, n)
            s["start"] = rng.integers(0, n_bases - 2000, n)
            s["group"] = rng.integers(0, n_groups, n)
            return s
        pav = h.pav(n_bases, n_groups)
        pav.import_(segs())
        t0 = time.perf_counter()
        pav.union()
        first = (time.perf_counter() - t0) * 1e3
        m = pav.counts()[1]
        pav.import_(segs())
        t0 = time.perf_counter()
        pav.union()
        second = (time.perf_counter() - t0) * 1e3
        m2 = pav.counts()[1]
        t0 = time.perf_counter()
        cells = pav.matrix(iv)
        matrix = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"segments": n, "union_ms": round(first, 3), "union_intervals": m, "second_union_of": m + n, "second_union_ms": round(second, 3),
                          "second_union_intervals": m2, "matrix_10000x8_ms": round(matrix, 3), "cells_sum": int(cells.sum())}), flush=True)
        pav.close()
    h.close()


if __name__ == "__main__":
    a = sys.argv
    if a[1] == "stage":
        stage(a[2], a[3], int(a[4]) if len(a) > 4 else 3, int(a[5]) if len(a) > 5 else 1000)
    else:
        union([int(x) for x in a[2:]])
