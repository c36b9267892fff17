"""What --genotypes costs (profiles/genotypes.md).  Three parts:

  ab TREE_A TREE_B PAIRS
                   `bench.py --gpus 1 --steps 10 --warmup 3` (C3, the switch off) of two built checkouts in fresh child processes, each
                   run from its own tree (its own capi.py, library and bench.py), A and B alternating, the order swapping from pair to
                   pair; one JSON line per run with ms_per_step.
  stage FASTA OUTDIR [REPS]
                   the command line end to end on FASTA all-vs-all (-p 90 -P 50k -t 16): without a switch, with --variants, with
                   --pav-window 1000, with --genotypes and with --genotypes --left-align, every mode once as warm-up, then REPS rounds
                   alternating, host clock around the child process; then one run of each with WFM_DEBUG=1, of which the lines of the
                   stages, of the device calls and of the finish are printed.  The PAF of every mode without --left-align is held against
                   the PAF without a switch, and the --variants file beside --genotypes against the one alone.
  table N [N ...]  a synthetic list of N variants (70 % SNVs, 15 % insertions, 15 % deletions of 1 .. 40 bases; one insertion of 70 000)
                   over 2.5e8 target bases and 8 groups, 20 000 = segments per group: host clock around add_variants and around
                   wfm_sites_table (both end in a synchronise), twice, with WFM_DEBUG=1 for the library's own lines.  Under
                   `rocprofv3 --kernel-trace --stats` (a run of its own) the kernels' times split the table call.
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


def ab(lib_a, lib_b, pairs):
    def run(tag, lib):
        tree = os.path.abspath(lib)
        env = {k: v for k, v in os.environ.items() if k not in ("WFM_LIB_PATH", "PYTHONPATH")}
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"],
                           capture_output=True, text=True, env=env, cwd=tree)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit("bench.py failed (%d) with %s: stopping" % (r.returncode, lib))
        d = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(json.dumps({"lib": tag, "ms_per_step": d.get("ms_per_step"), "cigar_identical_rate": d.get("cigar_identical_rate")}), flush=True)

    for k in range(pairs):
        for tag, lib in ((("A", lib_a), ("B", lib_b)) if k % 2 == 0 else (("B", lib_b), ("A", lib_a))):
            run(tag, lib)


MODES = [("off", []), ("variants", ["--variants", "{d}/{n}.vcf"]), ("pav", ["--pav-window", "1000", "--pav-out", "{d}/{n}.pav"]),
         ("genotypes", ["--genotypes", "{d}/{n}.gt.vcf"]), ("genotypes_left", ["--genotypes", "{d}/{n}.gt.vcf", "--left-align"]),
         ("both", ["--genotypes", "{d}/{n}.gt.vcf", "--variants", "{d}/{n}.vcf"])]
KEEP = ("[wflign] genotypes:", "[wflign] variants:", "[wflign] pav:", "[wfm] sites", "[wfm] pav", "[wfmash::align] genotypes:", "[wfmash::align] pav:",
        "[wfmash::genotypes]", "[wfmash::variants]", "[wfmash::pav]")


def stage(fa, outdir, reps):
    os.makedirs(outdir, exist_ok=True)

    def run(name, extra, debug=False):
        args = [CLI, "-p", "90", "-P", "50k", "-t", "16", "--out", os.path.join(outdir, name + ".paf")] + [x.format(d=outdir, n=name) for x in extra]
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

    for name, extra in MODES:
        run(name, extra)
    res = {name: [] for name, _ in MODES}
    for _ in range(reps):
        for name, extra in MODES:
            res[name].append(run(name, extra)[0])
    read = lambda n: open(os.path.join(outdir, n), "rb").read()
    plain = read("off.paf")
    gt = read("genotypes.gt.vcf").decode().splitlines()
    body = [l for l in gt if not l.startswith("#")]
    cells = "".join("".join(l.split("\t")[9:]) for l in body)
    print(json.dumps({"process_ms": res, "records": plain.count(b"\n"),
                      "paf_equal_to_off": {n: read(n + ".paf") == plain for n in ("variants", "pav", "genotypes", "both")},
                      "variants_file_equal_alone_and_beside": read("variants.vcf") == read("both.vcf"),
                      "genotypes_file_equal_alone_and_beside": read("genotypes.gt.vcf") == read("both.gt.vcf"),
                      "variant_lines": sum(1 for l in read("variants.vcf").splitlines() if not l.startswith(b"#")), "sites": len(body),
                      "sites_left_aligned": sum(1 for l in read("genotypes_left.gt.vcf").splitlines() if not l.startswith(b"#")),
                      "columns": gt[len(gt) - len(body) - 1].split("\t")[9:], "cells": {c: cells.count(c) for c in "01."},
                      "file_bytes": len(read("genotypes.gt.vcf"))}), flush=True)
    for name, extra in MODES[1:]:
        print("==== %s (WFM_DEBUG) ====" % name, flush=True)
        for line in run(name, extra, debug=True)[1].splitlines():
            if line.startswith(KEEP):
                print(line, flush=True)


def make_list(n, n_bases, n_groups):
    """n variants as an array of wfm_site_var_t and their allele bytes.  Positions lie on a grid of n / 3 places so that the groups meet on
    sites; the alleles of an SNV are a function of the place and of the group's parity (two ALTs per place); the bytes of the first
    200 000 indels are a function of the place, the others' of their index (distinct sites: the harder case for the sort)"""
    rng = np.random.default_rng(n)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    kind = rng.choice(np.array([0] * 14 + [1] * 3 + [2] * 3, dtype=np.uint32), size=n)
    gap = rng.integers(1, 41, size=n).astype(np.uint32)
    places = max(1, n // 3)
    v = np.zeros(n, dtype=capi.SITE_VAR_DTYPE)
    v["pos"] = rng.integers(0, places, size=n).astype(np.uint64) * np.uint64(max(1, (n_bases - 100000) // places))
    v["kind"] = kind
    v["group"] = rng.integers(0, n_groups, size=n)
    v["ref_len"] = np.where(kind == 2, gap + 1, 1)
    v["alt_len"] = np.where(kind == 1, gap + 1, 1)
    v["ref_len"][0], v["alt_len"][0], v["kind"][0] = 1, 70001, 1  # one insertion of 70 000 bases
    kind = v["kind"]
    lens = v["ref_len"].astype(np.int64) + v["alt_len"].astype(np.int64)
    first = np.concatenate(([0], np.cumsum(lens)[:-1]))
    v["off"] = first
    total = int(lens.sum())
    alleles = acgt[((np.arange(total, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(4)]
    alleles[first] = acgt[(v["pos"] % np.uint64(4)).astype(np.int64)]
    snv = kind == 0
    alleles[first[snv] + 1] = acgt[((v["pos"][snv] + np.uint64(1) + (v["group"][snv] % 2).astype(np.uint64)) % np.uint64(4)).astype(np.int64)]
    for k in np.flatnonzero(~snv)[:200000]:
        a, b = int(first[k]) + 1, int(first[k]) + int(lens[k])
        alleles[a:b] = acgt[(int(v["pos"][k]) + np.arange(b - a)) % 4]
    ins, dele = kind == 1, kind == 2
    alleles[first[ins] + 1] = alleles[first[ins]]  # an insertion's ALT begins with its anchor
    alleles[first[dele] + v["ref_len"][dele].astype(np.int64)] = alleles[first[dele]]  # a deletion's ALT is its anchor
    return v, alleles.tobytes()


def table(sizes):
    os.environ["WFM_DEBUG"] = "1"
    h = capi.Handle(0)
    n_bases, n_groups, seg = 250_000_000, 8, 20000
    for n in sizes:
        v, alleles = make_list(n, n_bases, n_groups)
        rng = np.random.default_rng(n + 1)
        obj = h.sites(n_bases, n_groups)
        probs = [(int(s), 0, 1, g) for g in range(n_groups) for s in rng.integers(0, n_bases - 6000, size=seg)]
        obj.add_ref(probs, [(5000 << 2) | 0])
        t0 = time.perf_counter()
        obj.add_variants(v, alleles)
        t_add = (time.perf_counter() - t0) * 1e3
        ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            sites, _, gt = obj.table()
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        c = obj.counts()
        print(json.dumps({"variants": n, "allele_bytes": len(alleles), "add_variants_ms": round(t_add, 2), "table_ms": ms, "sites": int(c[1]), "eq_intervals": int(c[2]),
                          "collisions": int(c[3]), "cells": {ch: int((gt == ord(ch)).sum()) for ch in "01."}}), flush=True)
        obj.close()
    h.close()


if __name__ == "__main__":
    a = sys.argv
    if a[1] == "ab":
        ab(a[2], a[3], int(a[4]))
    elif a[1] == "stage":
        stage(a[2], a[3], int(a[4]) if len(a) > 4 else 3)
    else:
        table([int(x) for x in a[2:]])
