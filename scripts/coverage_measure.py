"""What --coverage costs (profiles/coverage.md).  Two parts, one process:

  finish N_BASES   export + intervals of a synthetic difference array of N_BASES target bases (2e9: 8 GB) with sparse (LPA-like) and
                   with dense events, beside ONE plain device-to-device copy of the same bytes (torch, device events); then the
                   export -> import merge of 2 and of 4 objects on the one device.  The library's own WFM_DEBUG lines split a call
                   into the pass over the array and the rest; the host clock here is around the whole call, the copy into numpy included.
  stage LABEL FASTA MAPPING OUTDIR [REPS]
                   align_paf with the switch off / --coverage / --left-align --cs --variants / all four, alternating; host clock =
                   ms_total of the summary; then one pass each with WFM_DEBUG=1 for the stage lines.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wfmash_amd import capi  # noqa: E402


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return r, round((time.perf_counter() - t0) * 1e3, 2)


def fill(cov, n_bases, segments, seg_len, gap):
    """`segments` aligned stretches of seg_len bases, `gap` apart, as problems of 4096 runs of seg_len= gap D"""
    per, done, at = 2048, 0, 0
    words = np.empty(2 * per, dtype=np.uint32)
    words[0::2] = (seg_len << 2) | 0
    words[1::2] = (gap << 2) | 3
    span = per * (seg_len + gap)
    while done < segments and at + span <= n_bases:
        k = min(256, (segments - done + per - 1) // per, (n_bases - at) // span)
        if k == 0:
            break
        cov.add([(at + j * span, 0, 2 * per) for j in range(k)], words)
        done += k * per
        at += k * span
    return done


def finish(n_bases):
    import torch
    h = capi.Handle(0)
    os.environ["WFM_DEBUG"] = "1"
    for label, segments, seg_len, gap in (("sparse", 200_000, 3000, 5000), ("dense", 20_000_000, 30, 60)):
        cov = h.coverage(n_bases)
        done = fill(cov, n_bases, segments, seg_len, gap)
        for rep in range(3):
            e, ms_e = clock(cov.export)
            (iv, totals), ms_i = clock(cov.intervals)
            print(json.dumps({"finish": label, "n_bases": n_bases, "segments": done, "entries": len(e), "intervals": len(iv), "totals": totals,
                              "export_ms": ms_e, "intervals_ms": ms_i, "rep": rep}), flush=True)
        del e, iv
        cov.close()
    # the yardstick: one plain device-to-device copy of the array's bytes
    nbytes = (n_bases + 1) * 4
    a = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for rep in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps({"d2d_copy_bytes": nbytes, "ms": round(e0.elapsed_time(e1), 3), "rep": rep}), flush=True)
    del a, b
    torch.cuda.empty_cache()
    # the merge: k objects of the same device, each with its share of the sparse events, exported and imported into the first
    os.environ.pop("WFM_DEBUG")
    for k in (2, 4):
        handles = [h] + [capi.Handle(0) for _ in range(k - 1)]
        objs = [x.coverage(n_bases) for x in handles]
        for j, c in enumerate(objs):
            fill(c, n_bases, 200_000 // k, 3000, 5000 + 7 * j)
        for rep in range(2):
            t0 = time.perf_counter()
            moved = 0
            for c in objs[1:]:
                lst = c.export()
                objs[0].import_entries(lst)
                moved += len(lst)
            ms = round((time.perf_counter() - t0) * 1e3, 2)
            print(json.dumps({"merge_objects": k, "entries_moved": moved, "ms": ms, "rep": rep}), flush=True)
        for c in objs:
            c.close()
        for x in handles[1:]:
            x.close()
    h.close()


def stage(label, fa, paf, outdir, reps):
    h = capi.Handle(0)
    modes = [("off", False, False), ("coverage", True, False), ("la_cs_var", False, True), ("all", True, True)]

    def run(name, cover, rest):
        capi.set_coverage(os.path.join(outdir, "%s_%s.bg" % (label, name)) if cover else None)
        capi.set_left_align(rest)
        capi.set_cs(1 if rest else 0)
        capi.set_variants(os.path.join(outdir, "%s_%s.vcf" % (label, name)) if rest else None)
        out = os.path.join(outdir, "%s_%s.paf" % (label, name))
        s = capi.align_paf(h, fa, paf, out, params=dict(threads=16))
        counts = capi.coverage_counts()
        capi.set_coverage(None)
        capi.set_left_align(False)
        capi.set_cs(0)
        capi.set_variants(None)
        return dict(ms_total=round(s.ms_total, 2), written=int(s.written), batches=int(s.batches), coverage=counts)

    for m in modes:
        run(*m)
    res = {m[0]: [] for m in modes}
    for _ in range(reps):
        for m in modes:
            res[m[0]].append(run(*m))
    for name in res:
        print(json.dumps({"label": label, "mode": name, "ms_total": [r["ms_total"] for r in res[name]], "last": res[name][-1]}), flush=True)
    os.environ["WFM_DEBUG"] = "1"
    for m in modes[1:]:
        sys.stderr.write("==== %s %s (WFM_DEBUG) ====\n" % (label, m[0]))
        sys.stderr.flush()
        run(*m)
    h.close()


if __name__ == "__main__":
    if sys.argv[1] == "finish":
        finish(int(float(sys.argv[2])))
    else:
        stage(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5], int(sys.argv[6]) if len(sys.argv) > 6 else 3)
