"""Direct calls of wfm_cs_strings on C3's runs (64 pairs of 50 kb at 5 %), the seqset already on the device.  Usage: cs_direct.py FORM [CALLS]
Host clock per call (upload of the runs, two kernels, totals down, offsets up, strings down) and the bytes spelled."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wfmash_amd import capi, synth  # noqa: E402

form = int(sys.argv[1])
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
h = capi.Handle(0)
pairs = synth.pairs("C3", n_pairs=64)
S = h.upload([(p, t) for p, t in pairs])
failed, words = h.align_resident_rle(S)
assert failed == 0
for _ in range(3):
    strings, per = h.cs_strings(S, S.results, words, form)
ts = []
for _ in range(calls):
    t0 = time.perf_counter()
    strings, per = h.cs_strings(S, S.results, words, form)
    ts.append((time.perf_counter() - t0) * 1e3)
print(json.dumps({"form": "long" if form else "short", "problems": S.n, "runs": int(len(words)), "bytes": sum(len(s) for s in strings),
                  "ms_per_call_incl_python": [round(t, 3) for t in ts]}))
if os.environ.get("CS_DEBUG_PASS"):
    os.environ["WFM_DEBUG"] = "1"
    for _ in range(5):
        h.cs_strings(S, S.results, words, form)
S.free()
h.close()
