#!/usr/bin/env python3
"""Two builds of libwfmash_hip.so side by side on the align phase with every record pass on (profiles/emit_frame.md): the md5 of every
file and every switch's counts must be the same, and ms_total is reported per process.

    python scripts/emit_frame_ab.py --lib-a PARENT/libwfmash_hip.so --lib-b wfmash_amd/libwfmash_hip.so --out DIR [--procs 3] [--debug N]

tests/golden/LPA.subset.fa.gz against itself, the mapping rows as tests/test_transitive_driver_gpu.py makes them, a BED of five 1 kb
windows on the first sequence.  The switches: --cs=long, --maf, --variants, --coverage, --lift, --chain, --pav, --genotypes, --chain-net,
--transitive.  Every run is a fresh child process with WFM_LIB_PATH set, under a time limit of its own; a child starts only if the one
before it exited 0.  Each library is loaded once by a child that is not timed (profiles/driver_passes.md section 2 asks for it); then
A, B, A, B, ... `--procs` times each.  A child aligns the rows once without a switch, then once with all of them: the second run is the
timed one.  Then the child makes the six files an aligned PAF gives (--coverage-paf, --lift-paf, --chain-paf with --chain and with
--chain-net, --pav-paf, --transitive-paf) from the PAF it has just written, each call timed on the wall clock (profiles/paf_passes.md):
their md5 and out[4] are compared between the libraries as the run's are, and each is held against the run's own file.  --debug N: N more children each, alternating, with WFM_DEBUG=1, for the passes' own [wfm] lines."""
import argparse
import gzip
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
LPA = os.path.join(ROOT, "tests", "golden", "LPA.subset.fa.gz")
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")


def switches(capi):
    """name -> (set it for a run that writes `out` and reads `bed`, clear it, its counts)"""
    return {
        "cs": (lambda out, bed: capi.set_cs(2), lambda: capi.set_cs(0), capi.cs_counts),
        "maf": (lambda out, bed: capi.set_maf(out), lambda: capi.set_maf(None), capi.maf_counts),
        "variants": (lambda out, bed: capi.set_variants(out), lambda: capi.set_variants(None), capi.variants_counts),
        "coverage": (lambda out, bed: capi.set_coverage(out), lambda: capi.set_coverage(None), capi.coverage_counts),
        "lift": (lambda out, bed: capi.set_lift(bed, out), lambda: capi.set_lift(None, None), capi.lift_counts),
        "chain": (lambda out, bed: capi.set_chain(out), lambda: capi.set_chain(None), capi.chain_counts),
        "pav": (lambda out, bed: capi.set_pav(bed, 0, out), lambda: capi.set_pav(None, 0, None), capi.pav_counts),
        "genotypes": (lambda out, bed: capi.set_genotypes(out), lambda: capi.set_genotypes(None), capi.genotypes_counts),
        "chain_net": (lambda out, bed: capi.set_chain_net(out), lambda: capi.set_chain_net(None), capi.chain_net_counts),
        "transitive": (lambda out, bed: capi.set_transitive(bed, out, 2), lambda: capi.set_transitive(None, None), capi.transitive_counts),
    }


def child(workdir, tag, load_only):
    from wfmash_amd import capi
    capi.load()
    if load_only:
        print(json.dumps({"loaded": capi.LIB_PATH}), flush=True)
        return
    rows, bed = os.path.join(workdir, "map.paf"), os.path.join(workdir, "seeds.bed")
    h = capi.Handle(0)
    try:
        capi.align_paf(h, LPA, rows, os.path.join(workdir, tag + ".plain.paf"))
        sw = switches(capi)
        files = {n: os.path.join(workdir, tag + "." + n) for n in sw if n != "cs"}
        for n in sw:
            sw[n][0](files.get(n), bed)
        try:
            out = os.path.join(workdir, tag + ".paf")
            s = capi.align_paf(h, LPA, rows, out)
            counts = {n: [int(v) for v in sw[n][2]()] for n in sw}
        finally:
            for n in sw:
                sw[n][1]()
        files["paf"] = out
        offline = {"coverage": lambda o: capi.coverage_paf(h, LPA, out, o), "lift": lambda o: capi.lift_paf(h, LPA, out, bed, o),
                   "chain": lambda o: capi.chain_paf(h, LPA, out, o), "chain_net": lambda o: capi.chain_paf(h, LPA, out, None, net_path=o),
                   "pav": lambda o: capi.pav_paf(h, LPA, None, out, bed, 0, o), "transitive": lambda o: capi.transitive_paf(h, LPA, out, bed, o, depth=2)}
        offline_ms = {}
        for n, call in offline.items():
            files["offline." + n] = os.path.join(workdir, tag + ".offline." + n)
            t0 = time.perf_counter()
            counts["offline." + n] = [int(v) for v in call(files["offline." + n])]
            offline_ms[n] = round((time.perf_counter() - t0) * 1e3, 2)
        md5 = {n: hashlib.md5(open(p, "rb").read()).hexdigest() for n, p in sorted(files.items())}
        print(json.dumps({"library": capi.LIB_PATH, "ms_total": round(s.ms_total, 2), "ms_wflign": round(s.ms_wflign, 2), "ms_gpu": round(s.ms_gpu, 2),
                          "records": int(s.records), "written": int(s.written), "aligned_bp": int(s.aligned_bp), "batches": int(s.batches),
                          "md5": md5, "counts": counts, "offline_ms": offline_ms,
                          "offline_is_the_runs_file": all(md5["offline." + n] == md5[n] for n in offline)}, sort_keys=True), flush=True)
    finally:
        h.close()


def run_child(lib, workdir, tag, limit, load_only=False, debug_log=None):
    env = dict(os.environ, WFM_LIB_PATH=os.path.abspath(lib))
    env.pop("WFM_DEBUG", None)
    if debug_log:
        env["WFM_DEBUG"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", tag, "--out", workdir] + (["--load-only"] if load_only else [])
    r = subprocess.run(cmd, env=env, timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.PIPE if debug_log else None, text=True)
    if debug_log:
        with open(debug_log, "w") as f:
            f.write("".join(line + "\n" for line in r.stderr.splitlines() if line.startswith("[wfm]")))
    if r.returncode != 0:
        sys.exit(f"the run of {lib} ended with {r.returncode}: nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="TAG")
    ap.add_argument("--load-only", action="store_true")
    ap.add_argument("--lib-a")
    ap.add_argument("--lib-b")
    ap.add_argument("--out", default="emit_frame_ab_out")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--debug", type=int, default=0, metavar="N")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.out, a.child, a.load_only)
    a.out = os.path.abspath(a.out)
    os.makedirs(a.out, exist_ok=True)
    subprocess.check_call(["timeout", "-k", "10", str(a.limit), CLI, "-m", "-p", "90", "-P", "50k", "-t", "8", "--out", os.path.join(a.out, "map.paf"), LPA], cwd=a.out)
    name, length = None, 0
    for line in gzip.open(LPA, "rt"):
        if line.startswith(">"):
            if name:
                break
            name = line[1:].split()[0]
        else:
            length += len(line.strip())
    step = (length - 2000) // 5
    with open(os.path.join(a.out, "seeds.bed"), "w") as f:
        f.write("".join("%s\t%d\t%d\tw%d\n" % (name, 500 + k * step, 1500 + k * step, k) for k in range(5)))
    libs = (("parent", a.lib_a), ("branch", a.lib_b))
    for label, lib in libs:
        print(json.dumps(dict(run_child(lib, a.out, label, a.limit, load_only=True), label=label)), flush=True)
    runs = {label: [] for label, _ in libs}
    for k in range(a.procs):
        for label, lib in libs:
            r = run_child(lib, a.out, "%s%d" % (label, k), a.limit)
            runs[label].append(r)
            print(json.dumps(dict(r, label=label, process=2 * k + (label == "branch") + 1), sort_keys=True), flush=True)
    first = runs["parent"][0]
    same = all(r["md5"] == first["md5"] and r["counts"] == first["counts"] and r["written"] == first["written"] for rs in runs.values() for r in rs)
    ms = {label: sorted(r["ms_total"] for r in rs) for label, rs in runs.items()}
    lo, hi = ms["parent"][0], ms["parent"][-1]
    median = ms["branch"][len(ms["branch"]) // 2] if a.procs % 2 else (ms["branch"][a.procs // 2 - 1] + ms["branch"][a.procs // 2]) / 2
    inside = lo - (hi - lo) <= median <= hi + (hi - lo)
    for n in first["offline_ms"]:  # the same rule for the wall time of each of the six offline calls
        pm, bm = sorted(r["offline_ms"][n] for r in runs["parent"]), sorted(r["offline_ms"][n] for r in runs["branch"])
        med = bm[len(bm) // 2] if a.procs % 2 else (bm[a.procs // 2 - 1] + bm[a.procs // 2]) / 2
        print(json.dumps({"offline": n, "parent_ms": pm, "branch_ms": bm, "branch_median": med,
                          "parent_range_widened": [round(2 * pm[0] - pm[-1], 2), round(2 * pm[-1] - pm[0], 2)],
                          "inside": 2 * pm[0] - pm[-1] <= med <= 2 * pm[-1] - pm[0]}), flush=True)
    print(json.dumps({"files_and_counts_identical": same, "offline_is_the_runs_file": all(r["offline_is_the_runs_file"] for rs in runs.values() for r in rs),
                      "parent_ms_total": ms["parent"], "branch_ms_total": ms["branch"], "branch_median": median,
                      "parent_range_widened": [round(lo - (hi - lo), 2), round(hi + (hi - lo), 2)], "inside": inside}), flush=True)
    for k in range(a.debug):
        for label, lib in libs:
            run_child(lib, a.out, label + "_debug", a.limit, debug_log=os.path.join(a.out, "wfm_lines_%s_%d.log" % (label, k)))
    if not same:
        sys.exit("the two libraries differ in a file or a count")


if __name__ == "__main__":
    main()
