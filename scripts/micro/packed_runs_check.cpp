// packed_runs_check.cpp -- the two sources of packed runs (wfmash_amd/host/packed_runs.hpp) against each other: a record's ops packed as
// the align batch packs them, and the same record's PAF line -- spelled by the project's own writer -- parsed and packed as the --*-paf
// modes pack it, must be the same problem.  Then what the packing leaves out, and the reader's batches.  A program of its own, built with
// -fsanitize=address,undefined by tests/test_packed_runs_cpu.py and run directly; it needs no device and no library.
#include <cstdint>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "../../wfmash_amd/host/packed_runs.hpp"

namespace {

using wflign::CigarOps;
using wflign::PackedRuns;
using wflign::Place;

int failures = 0;
#define CHECK(cond, ...)                                                \
  do {                                                                  \
    if (!(cond)) {                                                      \
      ++failures;                                                       \
      fprintf(stderr, "packed_runs_check: %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                     \
      fprintf(stderr, "\n");                                            \
    }                                                                   \
  } while (0)

const uint64_t QSIZE = 5000, TSIZE = 7000, TARGET_OFF = 123456789012ull;

// a record of the align batch: its windows begin at (qoff, toff) and hold exactly the bases of its ops
struct Rec {
  CigarOps ops;
  uint64_t qoff = 0, qlen = 0, toff = 0, tlen = 0;
  bool rev = false;
};
Rec make_rec(const CigarOps& lead, const CigarOps& core, const CigarOps& trail, bool rev, uint64_t qoff, uint64_t toff) {
  Rec r;
  r.ops = lead;
  r.ops.insert(r.ops.end(), core.begin(), core.end());
  r.ops.insert(r.ops.end(), trail.begin(), trail.end());
  for (const auto& o : r.ops) {
    if (o.second != 'D') r.qlen += (uint64_t)o.first;
    if (o.second != 'I') r.tlen += (uint64_t)o.first;
  }
  r.rev = rev; r.qoff = qoff; r.toff = toff;
  return r;
}
chain::Record windows_of(const Rec& r) {
  chain::Record cr;
  cr.qname = "query#1"; cr.tname = "target#1"; cr.rev = r.rev;
  cr.qsize = QSIZE; cr.tsize = TSIZE;
  cr.qs = r.qoff; cr.qe = r.qoff + r.qlen; cr.ts = r.toff;
  return cr;
}
std::string line_of(const Rec& r) {
  wflign::PafParams pp;
  pp.min_identity = 0; pp.min_alignment_length = 0; pp.min_block_identity = 0;
  std::string line;
  const bool written = wflign::write_alignment_paf(line, r.ops, "query#1", QSIZE, r.qoff, r.qlen, r.rev, "target#1", TSIZE, r.toff, pp, 0.9f, 3, 2, 1);
  CHECK(written && !line.empty() && line.back() == '\n', "the writer wrote no line");
  if (!line.empty()) line.pop_back();
  return line;
}
int classify(const std::string& line, verify::Line& l) {
  const std::vector<uint64_t> lengths{TSIZE};
  int ti = -1;
  return coverage::classify_line(line, [](const std::string& name) { return name == "target#1" ? 0 : -1; }, lengths, l, &ti);
}

void same_problem(const char* what, const PackedRuns& a, const PackedRuns& b) {
  CHECK(a.size() == 1 && b.size() == 1 && a.where.size() == 1 && b.where.size() == 1 && a.place.size() == 1 && b.place.size() == 1, "%s: %zu and %zu problems",
        what, a.size(), b.size());
  if (a.size() != 1 || b.size() != 1) return;
  CHECK(a.probs[0].base == b.probs[0].base, "%s: base %llu, the line's %llu", what, (unsigned long long)a.probs[0].base, (unsigned long long)b.probs[0].base);
  CHECK(a.probs[0].runs_off == 0 && b.probs[0].runs_off == 0 && a.probs[0].n_runs == b.probs[0].n_runs && a.probs[0].n_runs == a.runs.size(), "%s: %u runs, the line's %u",
        what, a.probs[0].n_runs, b.probs[0].n_runs);
  CHECK(a.runs == b.runs, "%s: the run words differ", what);
  const chain::Record &x = a.where[0], &y = b.where[0];
  CHECK(x.qs == y.qs && x.qe == y.qe, "%s: query [%llu, %llu), the line's [%llu, %llu)", what, (unsigned long long)x.qs, (unsigned long long)x.qe,
        (unsigned long long)y.qs, (unsigned long long)y.qe);
  CHECK(x.ts == y.ts && x.te == y.te, "%s: target [%llu, %llu), the line's [%llu, %llu)", what, (unsigned long long)x.ts, (unsigned long long)x.te,
        (unsigned long long)y.ts, (unsigned long long)y.te);
  CHECK(x.qsize == y.qsize && x.tsize == y.tsize && x.rev == y.rev && x.qname == y.qname && x.tname == y.tname, "%s: sizes, strand or names differ", what);
  CHECK(a.place[0].target_off == b.place[0].target_off && a.place[0].group == b.place[0].group && a.place[0].query_world == b.place[0].query_world, "%s: places differ", what);
}

}  // namespace

int main() {
  // ---- the record side against the line side: every mix of I and D runs at both ends, both strands ----
  const std::vector<CigarOps> ends = {{}, {{3, 'I'}}, {{4, 'D'}}, {{3, 'I'}, {4, 'D'}}, {{4, 'D'}, {3, 'I'}}, {{2, 'I'}, {5, 'D'}, {1, 'I'}}};
  const CigarOps core = {{40, '='}, {2, 'X'}, {7, 'I'}, {11, '='}, {9, 'D'}, {1, 'X'}, {30, '='}};
  int cases = 0;
  for (const CigarOps& lead : ends)
    for (const CigarOps& trail : ends)
      for (int rev = 0; rev < 2; ++rev) {
        const Rec r = make_rec(lead, core, trail, rev != 0, 1000 + 17 * (uint64_t)cases, 2000 + 13 * (uint64_t)cases);
        char what[64];
        snprintf(what, sizeof what, "lead %zu, trail %zu, %c", lead.size(), trail.size(), rev ? '-' : '+');
        const Place place{5u, 777u, TARGET_OFF};
        PackedRuns from_ops, from_line;
        CHECK(wflign::pack_ops(from_ops, r.ops, windows_of(r), place) == 1, "%s: the record was not packed", what);
        verify::Line l;
        const int code = classify(line_of(r), l);
        CHECK(code == coverage::LINE_ADD, "%s: the reader makes \"%s\" of the writer's line", what, coverage::line_reason(code));
        if (code == coverage::LINE_ADD) wflign::pack_line(from_line, l, place);
        same_problem(what, from_ops, from_line);
        CHECK(from_ops.unknown == 0 && from_ops.runs.size() == core.size(), "%s: %zu runs of %zu", what, from_ops.runs.size(), core.size());
        ++cases;
      }
  // ---- what packs to nothing, and what is unknown: behind a record that is packed, so that a run left behind would show ----
  {
    PackedRuns pk;
    const Rec first = make_rec({}, core, {}, false, 10, 20);
    CHECK(wflign::pack_ops(pk, first.ops, windows_of(first), Place()) == 1, "the first record was not packed");
    const size_t n_runs = pk.runs.size();
    const Rec gaps = make_rec({{3, 'I'}}, {}, {{4, 'D'}, {2, 'I'}}, true, 10, 20);
    CHECK(wflign::pack_ops(pk, gaps.ops, windows_of(gaps), Place()) == 0, "a record of I and D alone was packed");
    CHECK(wflign::pack_ops(pk, CigarOps(), windows_of(gaps), Place()) == 0, "a record without ops was packed");
    CHECK(pk.size() == 1 && pk.runs.size() == n_runs && pk.unknown == 0, "a record of I and D alone left something behind");
    const std::vector<CigarOps> bad = {{{5, '='}, {0, 'X'}, {5, '='}}, {{5, '='}, {1 << 30, 'D'}, {5, '='}}, {{5, '='}, {-1, 'I'}, {5, '='}}, {{5, '='}, {3, 'M'}},
                                      {{2, 'I'}, {5, '='}, {2147483647, '='}, {2, 'D'}}};
    for (size_t k = 0; k < bad.size(); ++k) {
      const Rec r = make_rec({}, bad[k], {}, (k & 1) != 0, 10, 20);
      CHECK(wflign::pack_ops(pk, r.ops, windows_of(r), Place()) == -1, "bad record %zu is not unknown", k);
      CHECK(pk.unknown == k + 1 && pk.size() == 1 && pk.where.size() == 1 && pk.place.size() == 1 && pk.runs.size() == n_runs, "bad record %zu left something behind", k);
    }
    // the largest count the runs hold
    const Rec big = make_rec({}, {{(1 << 30) - 1, '='}}, {}, false, 0, 0);
    CHECK(wflign::pack_ops(pk, big.ops, windows_of(big), Place()) == 1 && pk.size() == 2 && pk.probs[1].runs_off == n_runs && pk.runs.back() == ((((1u << 30) - 1) << 2) | 0u),
          "a count of 2^30 - 1 was not packed");
  }
  // ---- the reader: the skip rules and their five counts, the hook, and a flush at exactly the limit ----
  {
    std::string text = "@HD\tnot a line\n\n";
    std::vector<std::string> good;
    for (int k = 0; k < 11; ++k) {
      const Rec r = make_rec(ends[(size_t)k % ends.size()], core, ends[(size_t)(k + 2) % ends.size()], (k & 1) != 0, 100 + 50 * (uint64_t)k, 300 + 70 * (uint64_t)k);
      good.push_back(line_of(r));
    }
    const std::string no_cg = good[0].substr(0, good[0].find("cg:Z:")) + "xx:i:1";
    std::string other_target = good[1], other_tlen = good[2], short_cigar = good[3];
    other_target.replace(other_target.find("target#1"), 8, "target#2");
    other_tlen.replace(other_tlen.find("\t7000\t"), 6, "\t7001\t");
    short_cigar.replace(short_cigar.find("cg:Z:"), std::string::npos, "cg:Z:5=");
    const std::vector<std::string> bad = {no_cg, other_target, other_tlen, short_cigar, "too\tfew\tfields"};
    for (size_t k = 0; k < good.size(); ++k) {
      text += good[k] + "\n";
      if (k < bad.size()) text += bad[k] + "\n";
    }
    const std::vector<uint64_t> lengths{TSIZE}, offsets{TARGET_OFF, TARGET_OFF + TSIZE};
    auto find = [](const std::string& name) { return name == "target#1" ? 0 : -1; };
    verify::Line fifth;  // the good line the hook leaves out
    CHECK(classify(good[4], fifth) == coverage::LINE_ADD, "the fifth good line is not taken");
    for (size_t limit = 1; limit <= 12; ++limit) {
      std::istringstream in(text);
      uint64_t skipped[5] = {0, 0, 0, 0, 0}, hooked = 0, taken = 0;
      std::vector<size_t> sizes;
      wflign::BatchLimits lim;
      lim.records = limit;
      wflign::read_packed_lines(in, find, lengths, offsets, lim, skipped,
                                [&](const verify::Line& l, Place& place) {
                                  CHECK(place.target_off == TARGET_OFF, "the hook sees target offset %llu", (unsigned long long)place.target_off);
                                  if (l.qs == fifth.qs && l.ts == fifth.ts) { ++hooked; return false; }
                                  place.group = (uint32_t)l.qs;
                                  return true;
                                },
                                [&](PackedRuns& pk) {
                                  CHECK(pk.order_base == taken, "limit %zu: order base %llu behind %llu lines", limit, (unsigned long long)pk.order_base, (unsigned long long)taken);
                                  CHECK(pk.where.size() == pk.size() && pk.place.size() == pk.size(), "limit %zu: lists of other lengths", limit);
                                  for (size_t j = 0; j < pk.size(); ++j) {
                                    CHECK(pk.place[j].group == (uint32_t)pk.where[j].qs, "limit %zu: the hook's place is not line %zu's", limit, j);
                                    CHECK(pk.probs[j].base == TARGET_OFF + pk.where[j].ts, "limit %zu: base of line %zu", limit, j);
                                    CHECK(pk.probs[j].runs_off + pk.probs[j].n_runs <= pk.runs.size() && (j == 0 ? pk.probs[j].runs_off == 0 : pk.probs[j].runs_off == pk.probs[j - 1].runs_off + pk.probs[j - 1].n_runs),
                                          "limit %zu: runs of line %zu", limit, j);
                                  }
                                  sizes.push_back(pk.size());
                                  taken += pk.size();
                                });
      CHECK(skipped[coverage::LINE_ADD] == 0 && skipped[coverage::LINE_NO_CIGAR] == 1 && skipped[coverage::LINE_MALFORMED] == 2 && skipped[coverage::LINE_UNKNOWN_TARGET] == 1 &&
                skipped[coverage::LINE_TLEN] == 1 && hooked == 1,
            "limit %zu: skipped %llu %llu %llu %llu %llu, hooked %llu", limit, (unsigned long long)skipped[0], (unsigned long long)skipped[1], (unsigned long long)skipped[2],
            (unsigned long long)skipped[3], (unsigned long long)skipped[4], (unsigned long long)hooked);
      CHECK(taken == 10 && sizes.size() == (10 + limit - 1) / limit, "limit %zu: %llu lines in %zu batches", limit, (unsigned long long)taken, sizes.size());
      for (size_t k = 0; k < sizes.size(); ++k)
        CHECK(sizes[k] == (k + 1 < sizes.size() || 10 % limit == 0 ? limit : 10 % limit), "limit %zu: batch %zu holds %zu lines", limit, k, sizes[k]);
    }
    // the limit of runs: a batch goes out with the line that reaches it
    {
      std::istringstream in(text);
      uint64_t skipped[5] = {0, 0, 0, 0, 0};
      std::vector<size_t> sizes;
      wflign::BatchLimits lim;
      lim.runs = 2 * core.size() + 1;
      wflign::read_packed_lines(in, find, lengths, offsets, lim, skipped, [](const verify::Line&, Place&) { return true; }, [&](PackedRuns& pk) { sizes.push_back(pk.size()); });
      CHECK(sizes == std::vector<size_t>({3, 3, 3, 2}), "the limit of runs: %zu batches", sizes.size());
    }
    const wflign::BatchLimits def;
    CHECK(def.records == 65536 && def.runs == ((size_t)16 << 20), "the limits are %zu problems and %zu runs", def.records, def.runs);
  }
  if (failures) return 1;
  printf("packed_runs_check: ok (%d records against their lines)\n", cases);
  return 0;
}
