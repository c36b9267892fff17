"""The score-only / score-limit surface as far as it can be checked without a device: the constants of include/wfmash_hip.h and their
Python twins, the flag bits through capi._make_problems, and a translation unit that uses the shim's AlignmentScope, setMaxAlignmentSteps
and the edit / gap-linear classes (tests/test_score_only_gpu.py runs it)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_USER = r'''
#include <cstdio>
#include <string>
#include "wfmash_amd/host/WFAligner.hpp"
int main(int argc, char** argv) {
  if (argc < 3) return 1;
  std::string target = argv[1], query = argv[2];
  wfa::WFAlignerGapAffine2Pieces scorer(0, 5, 8, 2, 24, 1, wfa::WFAligner::Score, wfa::WFAligner::MemoryUltralow);
  if (scorer.alignEnd2End(target, query) != 0) return 2;
  char* ops; int n;
  scorer.getAlignment(&ops, &n);
  printf("%d %d\n", scorer.getAlignmentScore(), n);
  scorer.setMaxAlignmentSteps(-scorer.getAlignmentScore() - 1);
  const int over = scorer.alignEnd2End(target, query);
  if (over != WF_STATUS_MAX_STEPS_REACHED || scorer.getAlignmentStatus() != wfa::WFAligner::StatusMaxStepsReached) return 3;
  printf("%d\n", over);
  scorer.setMaxAlignmentSteps(282);
  printf("%d\n", scorer.alignEnd2End(target, query));
  wfa::WFAlignerEdit edit(wfa::WFAligner::Score, wfa::WFAligner::MemoryUltralow);
  if (edit.alignEnd2End(target, query) != 0) return 4;
  printf("%d\n", edit.getAlignmentScore());
  wfa::WFAlignerGapLinear linear(4, 2, wfa::WFAligner::Alignment, wfa::WFAligner::MemoryHigh);
  (void)linear;
  return 0;
}
'''


def build_shim_user(tmp_path):
    src = tmp_path / "score_user.cpp"
    src.write_text(SHIM_USER)
    exe = tmp_path / "score_user"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + ROOT, str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "wfmash_amd"), "-lwfmash_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "wfmash_amd")])
    return str(exe)


def test_header_and_capi_agree_on_the_constants():
    from wfmash_amd import capi
    text = open(os.path.join(ROOT, "include", "wfmash_hip.h")).read()
    for name in ("WFM_MODE_MASK", "WFM_MODE_SCORE_ONLY", "WFM_MODE_SCORE_LIMIT", "WFM_ST_MAX_SCORE"):
        m = re.search(r"^#define\s+%s\s+\(?(-?(?:0x[0-9a-fA-F]+|\d+))\)?" % name, text, re.M)
        assert m, name
        assert int(m.group(1), 0) == getattr(capi, name), name
    assert (capi.WFM_MODE_MASK, capi.WFM_MODE_SCORE_ONLY, capi.WFM_MODE_SCORE_LIMIT, capi.WFM_ST_MAX_SCORE) == (0xff, 0x100, 0x200, -100)


def test_make_problems_carries_the_flag_bits():
    from wfmash_amd import capi
    so, lim = capi.WFM_MODE_SCORE_ONLY, capi.WFM_MODE_SCORE_LIMIT
    items = [(b"ACGT", b"ACGA"), (b"ACGT", b"ACGA", capi.WFM_MODE_END2END_BIWFA | so), (b"ACGT", b"ACGA", capi.WFM_MODE_ENDSFREE | so, 4, 0, 4, 0),
             (b"ACGT", b"ACGA", capi.WFM_MODE_END2END_BIWFA | so | lim, 0, 0, 0, 0, 17), (b"ACGT", b"ACGA", capi.WFM_MODE_END2END_UNI | so)]
    arr, keep, n = capi._make_problems(items)
    assert n == 5
    assert [arr[i].mode for i in range(n)] == [0, 0x100, 0x101, 0x300, 0x102]
    assert arr[3].score_hint == 17 and arr[2].pattern_begin_free == 4 and arr[2].text_begin_free == 4
    refs, _, _ = capi._make_refs([dict(pattern=b"ACGT", text=b"ACGA", mode=so | lim, score_hint=9)])
    assert refs[0].mode == 0x300 and refs[0].score_hint == 9


def test_score_shim_user_compiles_and_links(tmp_path):
    build_shim_user(tmp_path)


def test_tile_job_beyond_limit_at_the_edges():
    """wfa_plan.h: where the tile phase takes the limit for a verdict -- at a block that would begin at or past it, past half the bound
    (and the 64 of margin a direction), or where the bound leaves no diagonal; never without a limit."""
    import ctypes as C
    import numpy as np
    from wfmash_amd import capi
    L = capi._host()
    L.wfmh_test_rows.restype = C.c_int
    L.wfmh_test_rows.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    big, none = (5000, 5000), 1 << 29
    q = [(6,) + big + (300, 300, 200, 0),    # limit 300: the block from 200 is planned
         (6,) + big + (300, 300, 300, 0),    # none that begins at the limit
         (6,) + big + (1000, 1000, 564, 0),  # 2 s0 = bound + 128: goes on
         (6,) + big + (1000, 1000, 565, 0),  # past it: the verdict
         (6,) + big + (1000, 5000, 565, 0),  # the bound (a rigorous one below the limit) decides, not the limit
         (6,) + big + (10, 50, 35, 0),       # the bound as it stood 25 scores ago leaves diagonal 0
         (6,) + big + (10, 50, 36, 0),       # nothing left within the bound
         (6,) + big + (1000, 0, 900, 0),     # no limit: no verdict, whatever the bound
         (6,) + big + (none, 0, 10**6, 0),
         (7,) + big + (300, 300, 192, 0), (7,) + big + (300, 300, 320, 0)]
    qa = np.array(q, dtype=np.int32)
    out = np.zeros((len(q), 2), dtype=np.int64)
    assert L.wfmh_test_rows(qa.ctypes.data, len(q), out.ctypes.data) == 0
    assert out[:, 0].tolist() == [0, 1, 0, 1, 1, 0, 1, 0, 0, 0, 1]
