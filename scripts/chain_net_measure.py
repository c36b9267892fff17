"""What --chain-net costs (profiles/chain_net.md).  Four parts:

  ab TREE_A TREE_B PAIRS
                   `bench.py --gpus 1 --steps 10 --warmup 3` (C3, the switch off) of two built checkouts in fresh child processes, each
                   run from its own tree, A and B alternating, the order swapping from pair to pair; one JSON line per run.
  stage FASTA OUTDIR [REPS]
                   the command line end to end on FASTA all-vs-all (-p 90 -P 50k -t 16): without a switch, with --chain, with --chain-net,
                   with both and with --genotypes --left-align, every mode once as warm-up, then REPS rounds alternating, host clock around
                   the child process; then one run of each with WFM_DEBUG=1, of which the lines of the stages, of the device calls and of
                   the finish are printed.  The PAF of every mode without --left-align is held against the PAF without a switch, and the
                   --chain and --chain-net files beside each other against the ones alone.
  table N [N ...]  a synthetic list of N blocks of 100 bases at depth 8 (eight layers of blocks 125 bases apart, each layer shifted by 13
                   bases; a record is 50 consecutive blocks of a layer, its score drawn at random), and `pile`: 1000 records of 1000
                   blocks each over the same 125 000 bases.  Host clock around wfm_net_import and around wfm_net_table (both end in a
                   synchronise), three times, with WFM_DEBUG=1 for the library's own split of the table call.
  paint N [N ...]  the same lists on the host: NumPy, one cell per target base, painted block by block in ascending priority, then
                   the piece boundaries read off the cells -- what the device call is compared with.  No GPU.
"""
import ctypes as C
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


MODES = [("off", []), ("chain", ["--chain", "{d}/{n}.chain"]), ("net", ["--chain-net", "{d}/{n}.net.chain"]),
         ("both", ["--chain", "{d}/{n}.chain", "--chain-net", "{d}/{n}.net.chain"]), ("genotypes_left", ["--genotypes", "{d}/{n}.gt.vcf", "--left-align"])]
KEEP = ("[wflign] chain", "[wflign] genotypes:", "[wfm] net", "[wfm] chain", "[wfm] sites table", "[wfmash::align] chain-net:", "[wfmash::align] genotypes:",
        "[wfmash::chain", "[wfmash::genotypes]")


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
    print(json.dumps({"process_ms": res, "records": plain.count(b"\n"),
                      "paf_equal_to_off": {n: read(n + ".paf") == plain for n in ("chain", "net", "both")},
                      "chain_file_equal_alone_and_beside": read("chain.chain") == read("both.chain"),
                      "net_file_equal_alone_and_beside": read("net.net.chain") == read("both.net.chain"),
                      "chains": read("chain.chain").count(b"chain "), "net_chains": read("net.net.chain").count(b"chain "),
                      "chain_bytes": len(read("chain.chain")), "net_bytes": len(read("net.net.chain"))}), flush=True)
    for name, extra in MODES[1:]:
        print("==== %s (WFM_DEBUG) ====" % name, flush=True)
        for line in run(name, extra, debug=True)[1].splitlines():
            if line.startswith(KEEP):
                print(line, flush=True)


def make_list(n):
    """(blocks, recs, n_bases) of the synthetic list of n blocks; n == 'pile': the pile of depth 1000"""
    if n == "pile":
        per_rec, n_rec, layers = 1000, 1000, 1000
    else:
        per_rec, layers = 50, 8
        n_rec = max(layers, n // per_rec)
    in_layer = (n_rec + layers - 1) // layers  # records per layer
    rec = np.arange(n_rec, dtype=np.uint64)
    layer, place = rec % np.uint64(layers), rec // np.uint64(layers)
    k = np.arange(per_rec, dtype=np.uint64)
    t = ((place[:, None] * np.uint64(per_rec) + k[None, :]) * np.uint64(125) + layer[:, None] * np.uint64(13 if n != "pile" else 0)).reshape(-1)
    blocks = np.zeros(n_rec * per_rec, dtype=capi.NET_BLOCK_DTYPE)
    blocks["order"] = np.repeat(rec, per_rec)
    blocks["t"] = t
    blocks["q"] = np.tile((k * np.uint64(100)).astype(np.uint32), n_rec)
    blocks["size"] = 100
    recs = np.zeros(n_rec, dtype=capi.NET_REC_DTYPE)
    recs["order"] = rec
    recs["score"] = np.random.default_rng(n_rec).integers(0, 1 << 20, size=n_rec)
    return blocks, recs, int(in_layer * per_rec * 125 + 13 * layers + 200)


def table(sizes):
    os.environ["WFM_DEBUG"] = "1"
    h = capi.Handle(0)
    for n in sizes:
        blocks, recs, n_bases = make_list(n)
        obj = h.net(n_bases)
        t0 = time.perf_counter()
        obj.import_(blocks, recs)
        t_add = (time.perf_counter() - t0) * 1e3
        ms = []
        f = obj._L.wfm_net_table
        for _ in range(3):
            pp, rp, np_, nr = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
            t0 = time.perf_counter()
            rc = f(h._p, obj._p, C.byref(pp), C.byref(np_), C.byref(rp), C.byref(nr))
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            if rc != 0:
                raise SystemExit("wfm_net_table failed (%d): %s" % (rc, h.last_error()))
            obj._L.wfm_net_free_list(pp)
            obj._L.wfm_net_free_list(rp)
        c = obj.counts()
        print(json.dumps({"blocks": len(blocks), "records": len(recs), "n_bases": n_bases, "import_ms": round(t_add, 2), "table_ms": ms, "intervals": c[2],
                          "pieces": c[3], "won_nothing": c[4]}), flush=True)
        obj.close()
    h.close()


def paint(sizes):
    for n in sizes:
        blocks, recs, n_bases = make_list(n)
        t0 = time.perf_counter()
        # priority: score descending, order ascending; the worst first
        rank = np.lexsort((-recs["order"].astype(np.int64), recs["score"]))
        prio = np.empty(len(recs), dtype=np.int64)
        prio[rank] = np.arange(len(recs))
        by = np.argsort(prio[blocks["order"].astype(np.int64)], kind="stable")
        owner = np.full(n_bases, -1, dtype=np.int32)
        ts, sz = blocks["t"].astype(np.int64), blocks["size"].astype(np.int64)
        for b in by:
            owner[ts[b]:ts[b] + sz[b]] = b
        heads = np.flatnonzero((owner >= 0) & (np.concatenate(([-2], owner[:-1])) != owner))
        ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"blocks": len(blocks), "records": len(recs), "n_bases": n_bases, "host_paint_ms": round(ms, 1), "pieces": int(len(heads))}), flush=True)


if __name__ == "__main__":
    a = sys.argv
    size = lambda x: x if x == "pile" else int(x)
    if a[1] == "ab":
        ab(a[2], a[3], int(a[4]))
    elif a[1] == "stage":
        stage(a[2], a[3], int(a[4]) if len(a) > 4 else 3)
    elif a[1] == "table":
        table([size(x) for x in a[2:]])
    else:
        paint([size(x) for x in a[2:]])
