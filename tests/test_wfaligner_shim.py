"""The wfa::WFAligner shim (seam 1 of INTEGRATION.md): a translation unit written like the
reference's call sites (wflign.cpp:136-165, 280-309) must compile against it and, on a GPU box,
produce the oracle's op strings."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include <cstdio>
#include <cstring>
#include <string>
#include "wfmash_amd/host/WFAligner.hpp"
int main(int argc, char** argv) {
  std::string target = argv[1], query = argv[2];
  wfa::WFAlignerGapAffine2Pieces wf_aligner(0, 5, 8, 2, 24, 1, wfa::WFAligner::Alignment, wfa::WFAligner::MemoryUltralow);
  wf_aligner.setHeuristicNone();
  const int status = wf_aligner.alignEnd2End(target.data(), (int)target.size(), query.data(), (int)query.size());
  if (status != 0) return 2;
  char* ops; int n;
  wf_aligner.getAlignment(&ops, &n);
  printf("%.*s\n", n, ops);
  wfa::WFAlignerGapAffine2Pieces head(0, 5, 8, 2, 24, 1, wfa::WFAligner::Alignment, wfa::WFAligner::MemoryMed);
  std::string hq = query.substr(0, 60), ht = target.substr(0, 64);
  if (head.alignEndsFree(ht, (int)ht.size(), 0, hq, (int)hq.size(), 0) != 0) return 3;
  printf("%s\n", head.getAlignment().c_str());
  return 0;
}
'''


# alignEndsFree with any four free lengths, in both scopes: per scope one line "status score ops_len", then the status under each limit
SRC_ENDSFREE = r'''
#include <cstdio>
#include <cstdlib>
#include <string>
#include "wfmash_amd/host/WFAligner.hpp"
int main(int argc, char** argv) {
  if (argc < 7) return 1;
  std::string pattern = argv[1], text = argv[2];
  const int pbf = atoi(argv[3]), pef = atoi(argv[4]), tbf = atoi(argv[5]), tef = atoi(argv[6]);
  const wfa::WFAligner::AlignmentScope scopes[2] = {wfa::WFAligner::Alignment, wfa::WFAligner::Score};
  for (int s = 0; s < 2; ++s) {
    wfa::WFAlignerGapAffine2Pieces a(0, 5, 8, 2, 24, 1, scopes[s], wfa::WFAligner::MemoryMed);
    a.setHeuristicNone();
    const int st = a.alignEndsFree(pattern, pbf, pef, text, tbf, tef);
    printf("%d %d %d\n", st, a.getAlignmentScore(), (int)a.getAlignment().size());
    for (int i = 7; i < argc; ++i) {
      a.setMaxAlignmentSteps(atoi(argv[i]));
      const int lst = a.alignEndsFree(pattern, pbf, pef, text, tbf, tef);
      printf("%d %d\n", lst, a.getAlignmentStatus());
    }
  }
  return 0;
}
'''


def _build(tmp_path, text=SRC, name="shim_user"):
    src = tmp_path / (name + ".cpp")
    src.write_text(text)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + ROOT, str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "wfmash_amd"), "-lwfmash_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "wfmash_amd")])
    return str(exe)


def test_shim_compiles_and_links(tmp_path):
    _build(tmp_path)
    _build(tmp_path, SRC_ENDSFREE, "shim_endsfree")


@pytest.mark.gpu
def test_shim_endsfree_score_and_step_limit_are_the_same_in_both_scopes(tmp_path, oracle):
    """alignEndsFree with partial free lengths: getAlignmentScore() is minus the oracle's ends-free score in Alignment and in Score scope,
    and setMaxAlignmentSteps means the same in both -- a limit between the ends-free score and the price of the op string's runs (which
    counts the free end gaps) lets the call complete, a limit below the ends-free score ends it WF_STATUS_MAX_STEPS_REACHED."""
    from wfmash_amd import synth
    import endsfree_cases
    core = synth.random_dna(0x5A1, 300)
    p = core
    t = synth.random_dna(0x5A2, 80) + synth.mutate(core, 0.05, 0x5A3) + synth.random_dna(0x5A4, 60)
    free = (0, 0, 90, 50)  # the junk in front is covered, ten bases of the junk behind are paid
    rc, ops, sc, _ = oracle.align_endsfree(p, free[0], free[1], t, free[2], free[3])
    assert rc == 0 and sc == oracle.dp_score_endsfree(p, t, *free) == endsfree_cases.endsfree_price(ops, free)
    by_runs = oracle.ops_score(ops)
    assert 0 < sc < by_runs - 1
    between, below = (sc + by_runs) // 2, sc - 1
    exe = _build(tmp_path, SRC_ENDSFREE, "shim_endsfree")
    out = subprocess.check_output([exe, p.decode(), t.decode()] + [str(x) for x in free + (between, sc, below)]).decode().split("\n")
    for scope, lines in (("Alignment", out[0:4]), ("Score", out[4:8])):
        assert lines[0] == "0 %d %d" % (-sc, len(ops) if scope == "Alignment" else 0), (scope, lines[0], sc, by_runs)
        assert lines[1] == "0 0" and lines[2] == "0 0", (scope, lines)  # within the limit, and exactly at it
        assert lines[3] == "-100 -100", (scope, lines)


@pytest.mark.gpu
def test_shim_matches_oracle(tmp_path, oracle):
    from wfmash_amd import synth
    exe = _build(tmp_path)
    t = synth.random_dna(77, 700)
    q = synth.mutate(t, 0.06, 78)
    out = subprocess.check_output([exe, t.decode(), q.decode()]).decode().split("\n")
    rc, ops, _, _ = oracle.align_biwfa(t, q)
    assert out[0].encode() == ops
    rc, hops, _, _ = oracle.align_endsfree(t[:64], 64, 0, q[:60], 60, 0)
    assert out[1].encode() == hops
