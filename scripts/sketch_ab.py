#!/usr/bin/env python3
"""A/B of two builds of libwfmash_hip.so on a fixed battery of sketch calls: the minmer records, the per-sequence counts,
the return values and every integer of the two WFM_DEBUG lines of build B must be those of build A.  Made for changes of the
sketch pipeline (host/minmers.cpp, add_minmers_core) that must not change a byte.

    python scripts/sketch_ab.py --lib-a OLD/libwfmash_hip.so --lib-b wfmash_amd/libwfmash_hip.so --out DIR

Every run is a fresh child process that names its library with WFM_LIB_PATH (capi.py loads that one), one per library and per
case, under `timeout -k 10`; a child starts only if the one before it exited 0.  Build A runs twice first: a field that differs
between those two runs is unstable by itself, is listed, and is left out of the comparison -- only the millisecond figures of
the debug lines may be among them.  Then B runs, and what is left of its fields has to equal A's.

The cases (tests/test_minmers.py has the lists):
  mixed            _mixed_routes() as its test runs it: k, w, s = 15, 256, 12, 8 threads, WFM_WINNOW_CHUNK=16384, WFM_WINNOW_DEV_MIN=50000
  finish_host      the same with WFM_FINISH_DEVICE=0
  no_device        ... WFM_WINNOW_DEVICE=0
  force1, force2   ... WFM_WINNOW_FORCE=1 / 2
  no_prefilter     ... WFM_PREFILTER=0
  one_thread       ... threads=1
  thin             _thin_cases() at (15, 1000, 39), WFM_WINNOW_CHUNK=64000, WFM_WINNOW_DEV_MIN=0
  production       one 5.5 Mbp sequence with no switch set: the production thresholds
  part             wfm_sketch_part on the mixed list (the device sink): offs and the downloaded records
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MIXED = {"WFM_WINNOW_CHUNK": "16384", "WFM_WINNOW_DEV_MIN": "50000"}
# name -> (list, (k, w, s), threads, environment)
CASES = {
    "mixed": ("mixed", (15, 256, 12), 8, MIXED),
    "finish_host": ("mixed", (15, 256, 12), 8, dict(MIXED, WFM_FINISH_DEVICE="0")),
    "no_device": ("mixed", (15, 256, 12), 8, dict(MIXED, WFM_WINNOW_DEVICE="0")),
    "force1": ("mixed", (15, 256, 12), 8, dict(MIXED, WFM_WINNOW_FORCE="1")),
    "force2": ("mixed", (15, 256, 12), 8, dict(MIXED, WFM_WINNOW_FORCE="2")),
    "no_prefilter": ("mixed", (15, 256, 12), 8, dict(MIXED, WFM_PREFILTER="0")),
    "one_thread": ("mixed", (15, 256, 12), 1, MIXED),
    "thin": ("thin", (15, 1000, 39), 8, {"WFM_WINNOW_CHUNK": "64000", "WFM_WINNOW_DEV_MIN": "0"}),
    "production": ("long", (15, 1000, 39), 8, {}),
    "part": ("mixed", (15, 256, 12), 8, MIXED),
}


def sequences(which):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from wfmash_amd import synth
    import test_minmers
    if which == "mixed":
        return test_minmers._mixed_routes()
    if which == "thin":
        return [s for _, s in test_minmers._thin_cases() if len(s) >= 1000]
    b = bytearray(synth.random_dna(0x3a3, 5_500_000))
    b[1_000_000:1_020_000] = b"N" * 20_000
    b[2_000_000:2_030_000] = (bytes(b[100:107]) * 5000)[:30_000]
    b[3_000_000:3_048_000] = bytes(b[5000:6200]) * 40
    return [bytes(b)]


def child(name, dump_path):
    """one case through the library WFM_LIB_PATH names; the records as one digest per sequence"""
    import ctypes as C
    import numpy as np
    from wfmash_amd import capi
    which, (k, w, s), threads, _ = CASES[name]
    seqs = sequences(which)
    h = capi.Handle(0)
    try:
        if name == "part":
            part = h.sketch_part(seqs, k, w, s, threads=threads)
            tot, counts = part.info()
            recs = part.download()
            part.free()
        else:  # (capi's add_minmers_multi does not pass the return value on)
            n = len(seqs)
            ids = np.arange(n, dtype=np.int32)
            bufs = [np.frombuffer(x, dtype=np.uint8) for x in seqs]
            ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
            lens = np.array([len(x) for x in seqs], dtype=np.int64)
            cap = 4 * int(lens.sum()) + 64
            out = np.zeros(cap, dtype=capi.MINMER_DTYPE)
            counts = np.zeros(n, dtype=np.int64)
            f = h._L.wfm_add_minmers_multi
            f.restype = C.c_int64
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
            tot = f(h._p, ptrs, lens.ctypes.data, ids.ctypes.data, n, k, w, s, threads, out.ctypes.data, cap, counts.ctypes.data)
            offs = np.concatenate([[0], np.cumsum(counts)])
            recs = [out[offs[i]:offs[i + 1]] for i in range(n)]
    finally:
        h.close()
    dump = {"library": capi.load()._name, "return": int(tot), "counts": [int(c) for c in counts],
            "records": [hashlib.sha256(r.tobytes()).hexdigest() for r in recs], "record_bytes": sum(r.nbytes for r in recs)}
    with open(dump_path, "w") as f:
        json.dump(dump, f, sort_keys=True)
    print(f"case {name}: returned {tot}, {len(counts)} sequences", flush=True)


def debug_fields(stderr):
    """the two [wfm] lines: their integers (and the kept share) apart from their millisecond figures"""
    out = {}
    for tag, key in (("winnowing on the device:", "device_line"), ("add_minmers_multi:", "multi_line")):
        lines = [l for l in stderr.splitlines() if tag in l]
        out[key + ".count"] = len(lines)
        for j, l in enumerate(lines):
            l = l.split(tag)[1]
            out[f"{key}.{j}.ms"] = re.findall(r"\d+\.\d+ ms", l) + re.findall(r"\((?:GPU hashing|longest stitch) \d+\.\d+|thinning \d+\.\d+", l)
            rest = re.sub(r"\d+\.\d+ ms|(GPU hashing|longest stitch|thinning) \d+\.\d+", "", l)
            out[f"{key}.{j}.kept_share"] = re.findall(r"\d+\.\d+ %", rest)
            out[f"{key}.{j}.ints"] = re.findall(r"0x[0-9a-f]+|\d+", re.sub(r"\d+\.\d+ %", "", rest))
            out[f"{key}.{j}.where"] = [x for x in ("on the device", "on the host", "streamed through the pinned ring", "whole sequences") if x in l]
    return out


def run_children(lib, tag, outdir, limit):
    """one child per case -> {(case, field): value}"""
    fields = {}
    for name, (_, _, _, switches) in CASES.items():
        dump_path = os.path.join(outdir, f"{tag}_{name}.json")
        env = {k: v for k, v in os.environ.items() if not k.startswith(("WFM_WINNOW", "WFM_PREFILTER")) and k not in ("WFM_FINISH_DEVICE", "WFM_LIB")}
        env.update(switches, WFM_LIB_PATH=os.path.abspath(lib), WFM_DEBUG="1")
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", name, "--dump", dump_path]
        r = subprocess.run(cmd, env=env, stderr=subprocess.PIPE, text=True)
        with open(os.path.join(outdir, f"{tag}_{name}.stderr"), "w") as f:
            f.write(r.stderr)
        if r.returncode != 0:
            sys.exit(f"the run of {lib} (case {name}) ended with {r.returncode}: nothing more is started\n{r.stderr[-2000:]}")
        d = json.load(open(dump_path))
        if os.path.abspath(d.pop("library")) != os.path.abspath(lib):
            sys.exit(f"case {name} loaded another library than {lib}")
        d.update(debug_fields(r.stderr))
        for k, v in d.items():
            fields[(name, k)] = v
    return fields


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="CASE")
    ap.add_argument("--dump")
    ap.add_argument("--lib-a")
    ap.add_argument("--lib-b")
    ap.add_argument("--out", default="sketch_ab_out")
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.dump)
    os.makedirs(a.out, exist_ok=True)
    a1 = run_children(a.lib_a, "a1", a.out, a.limit)
    if not all(a1[(c, "return")] > 0 and a1[(c, "multi_line.count")] == 1 for c in CASES) or a1[("mixed", "device_line.count")] != 1:
        sys.exit("build A: a case made no record or wrote no debug line")
    a2 = run_children(a.lib_a, "a2", a.out, a.limit)
    unstable = sorted({k for k in a1 if a1[k] != a2.get(k)})
    print("unstable between two runs of A (left out):", [f"{c}:{f}" for c, f in unstable] or "none")
    if any(not f.endswith(".ms") for _, f in unstable):
        sys.exit("a field that is no time differs between two runs of the same library")
    b = run_children(a.lib_b, "b", a.out, a.limit)
    diff = sorted(f"{c}:{f}" for (c, f) in set(a1) | set(b) if (c, f) not in unstable and not f.endswith(".ms") and a1.get((c, f)) != b.get((c, f)))
    kept = [k for k in a1 if k not in unstable and not k[1].endswith(".ms")]
    print(f"compared {len(kept)} fields of {len(CASES)} cases, {sum(a1[(c, 'record_bytes')] for c in CASES)} bytes of records")
    if diff:
        sys.exit("B differs from A in: " + ", ".join(diff))
    print("A/B identical")


if __name__ == "__main__":
    main()
