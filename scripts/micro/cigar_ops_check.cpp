// cigar_ops_check.cpp -- the align path's CIGAR helpers (wfmash_amd/host/cigar_ops.hpp) on random inputs, for the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined scripts/micro/cigar_ops_check.cpp -o cigar_ops_asan && ./cigar_ops_asan
//
// Over random CIGARs, with bases made to fit them: erode, merge_adjacent_ops and merge_cigar_ops keep the query and target lengths;
// the scans erode whole runs from their end and stop by the one rule; plan_patches is the two scans and its independence rule
// holds against a random head patch; after a swap no two neighbours share an op and the '=' + 'D' target length is what it was;
// the PAF writer's cg:Z: field parses back to the trimmed runs and the SAM writer's SEQ and MD:Z fit them.  Exit status 0 = all held.
#include <cstdio>
#include <random>

#include "../../wfmash_amd/host/cigar_ops.hpp"

using namespace wflign;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s (CIGAR %ld: %s)\n", __FILE__, __LINE__, #c, it, cigar_to_string(ops).c_str()); return 1; } } while (0)

static std::mt19937_64 rng(2026);
static int64_t below(uint64_t n) { return (int64_t)(rng() % n); }

static CigarOps random_ops(int n_runs, const char* alphabet, int n_alpha, bool long_runs) {
  CigarOps ops;
  char prev = 0;
  for (int i = 0; i < n_runs; ++i) {
    char op;
    do op = alphabet[below((uint64_t)n_alpha)]; while (op == prev && n_alpha > 1);
    const int lens[] = {1, 1, 2, 3, 3, 4, 11, 12, 1 + (int)below(40), 100 + (int)below(300)};
    ops.emplace_back(lens[below(long_runs ? 10 : 9)], op);
    prev = op;
  }
  return ops;
}
static void lengths(const CigarOps& ops, uint64_t& q, uint64_t& t, uint64_t* eq_del_t = nullptr) {
  q = t = 0;
  uint64_t ed = 0;
  for (const auto& o : ops) {
    if (o.second == '=' || o.second == 'X' || o.second == 'M') { q += (uint64_t)o.first; t += (uint64_t)o.first; }
    else if (o.second == 'I') q += (uint64_t)o.first;
    else if (o.second == 'D') t += (uint64_t)o.first;
    if (o.second == '=' || o.second == 'D') ed += (uint64_t)o.first;
  }
  if (eq_del_t) *eq_del_t = ed;
}
static bool neighbours_differ(const CigarOps& ops) {
  for (size_t i = 1; i < ops.size(); ++i) if (ops[i].second == ops[i - 1].second) return false;
  return true;
}
// bases that fit the CIGAR ('=' equal, 'X' different), from a two-letter alphabet so that runs can slide across gaps
static void make_bases(const CigarOps& ops, std::string& q, std::string& t) {
  q.clear(); t.clear();
  for (const auto& o : ops)
    for (int j = 0; j < o.first; ++j) {
      const char c = "AC"[below(2)];
      if (o.second == '=' || o.second == 'M') { q += c; t += c; }
      else if (o.second == 'X') { q += c; t += (c == 'A' ? 'C' : 'A'); }
      else if (o.second == 'I') q += c;
      else t += c;
    }
}

int main() {
  long it = 0, eroded = 0, swaps_start = 0, swaps_end = 0, independent = 0, later = 0, paf = 0, sam = 0;
  for (it = 0; it < 300000; ++it) {
    const bool eq_del_only = it % 3 == 0;  // (the end swap takes nothing else)
    CigarOps ops = eq_del_only ? random_ops(1 + (int)below(8), "=D", 2, it % 2) : random_ops(1 + (int)below(it % 50 == 0 ? 60 : 14), "=XID", 4, it % 5 < 3);
    uint64_t q0, t0, q1, t1;
    lengths(ops, q0, t0);

    // erode, on either end; merge_adjacent_ops; merge_cigar_ops
    for (int head = 0; head < 2; ++head) {
      CigarOps e = ops;
      const bool changed = erode_short_matches_in_cigar(e, 3, head != 0);
      lengths(e, q1, t1);
      CHECK(q1 == q0 && t1 == t0 && (changed || e == ops) && (!changed || (e.size() < ops.size() && neighbours_differ(e))));
      eroded += changed;
    }
    {
      const CigarOps other = random_ops((int)below(6), "=XID", 4, true);
      uint64_t q2, t2;
      lengths(other, q2, t2);
      CigarOps m = ops;
      const size_t from = other.empty() ? 0 : (size_t)below(other.size()), to = from + (other.empty() ? 0 : (size_t)below(other.size() - from + 1));
      merge_adjacent_ops(m, other, 0, other.size());
      lengths(m, q1, t1);
      CHECK(q1 == q0 + q2 && t1 == t0 + t2 && m.size() + 1 >= ops.size() + other.size() && neighbours_differ(m));
      CigarOps part = ops;
      merge_adjacent_ops(part, other, from, to);
      CHECK(part.size() + 1 >= ops.size() + (to - from) && part.size() <= ops.size() + (to - from));
      CigarOps twice = ops;
      twice.insert(twice.end(), ops.begin(), ops.end());
      merge_cigar_ops(twice);
      lengths(twice, q1, t1);
      CHECK(q1 == 2 * q0 && t1 == 2 * t0 && neighbours_differ(twice));
    }

    // the scans and the plan
    size_t looked = ~(size_t)0;
    const Erosion he = scan_head_erosion(ops), te = scan_tail_erosion(ops, &looked);
    {
      uint64_t q = 0, t = 0;
      lengths(CigarOps(ops.begin(), ops.begin() + (long)he.erode_end_pos), q, t);
      CHECK(he.erode_end_pos <= ops.size() && q == he.query_eroded && t == he.target_eroded);
      lengths(CigarOps(ops.begin() + (long)te.erode_start_idx, ops.end()), q, t);
      CHECK(te.erode_start_idx <= ops.size() && q == te.query_eroded && t == te.target_eroded);
      CHECK(looked == te.erode_start_idx || looked + 1 == te.erode_start_idx);
      CHECK(he.erode_end_pos >= 1 && te.erode_start_idx + 1 <= ops.size());  // the first run always goes
      const PatchPlan pl = plan_patches(ops);
      CHECK(pl.head.erode_end_pos == he.erode_end_pos && pl.tail.erode_start_idx == te.erode_start_idx && pl.head_wanted == patch_wanted(he) &&
            pl.tail_wanted == patch_wanted(te) && pl.tail_independent == (!pl.head_wanted || looked > he.erode_end_pos));
      if (pl.head_wanted && pl.tail_independent) {
        CigarOps patched = random_ops(1 + (int)below(7), "=XID", 4, true);
        merge_adjacent_ops(patched, ops, he.erode_end_pos, ops.size());
        const Erosion te2 = scan_tail_erosion(patched);
        CHECK(te2.query_eroded == te.query_eroded && te2.target_eroded == te.target_eroded &&
              patched.size() - te2.erode_start_idx == ops.size() - te.erode_start_idx &&
              std::equal(patched.begin() + (long)te2.erode_start_idx, patched.end(), ops.begin() + (long)te.erode_start_idx));
        ++independent;
      } else later += pl.head_wanted;
    }

    // the swaps, on bases that fit the CIGAR and on bases cut short
    std::string q, t;
    make_bases(ops, q, t);
    uint64_t ed0, ed1;
    lengths(ops, q1, t1, &ed0);
    for (int cut = 0; cut < 2; ++cut) {
      const int64_t qn = (int64_t)q.size() - (cut ? below(q.size() + 1) : 0), tn = (int64_t)t.size() - (cut ? below(t.size() + 1) : 0);
      CigarOps s = ops;
      const bool a = try_swap_start_pattern(s, q.data(), qn, t.data(), tn);
      lengths(s, q1, t1, &ed1);
      CHECK(q1 == q0 && t1 == t0 && ed1 == ed0 && (a ? neighbours_differ(s) : s == ops));
      CigarOps s2 = s;
      const bool b = try_swap_end_pattern(s2, q.data(), qn, t.data(), tn);
      lengths(s2, q1, t1, &ed1);
      CHECK(q1 == q0 && t1 == t0 && ed1 == ed0 && (b ? neighbours_differ(s2) : s2 == s));
      swaps_start += a; swaps_end += b;
    }

    // the writers
    {
      PafParams pp;
      std::string line;
      RecordCore c;
      const bool kept = trim_and_filter(ops, 1000, 5000000000ull, pp, c);
      CHECK(c.b <= c.e && c.e <= ops.size());
      const bool rev = it % 2;
      CHECK(write_alignment_paf(line, ops, "q#1", 5000000000ull + q0 + 7, 5000000000ull, q0, rev, "t#1", 1000 + t0 + 9, 1000, pp, 0.95f, 3, it % 4 ? 2 : 0, 1) == kept);
      if (kept) {
        CHECK(line.back() == '\n' && line.find("\t\t") == std::string::npos);
        const size_t cg = line.find("cg:Z:");
        CHECK(cg != std::string::npos && parse_cigar(line.substr(cg + 5, line.size() - cg - 6)) == CigarOps(ops.begin() + (long)c.b, ops.begin() + (long)c.e));
        ++paf;
      }
      std::string rec;
      CHECK(write_alignment_sam(rec, ops, "q#1", 5000000000ull, rev, "t#1", 1000, pp, 0.95f, it % 3 == 0, true, q.data(), t.data(), 3, 2, 1) == kept);
      if (kept) {
        CHECK(rec.back() == '\n' && rec.find("\tMD:Z:") != std::string::npos && rec.find(cigar_to_string(ops, c.b, c.e)) != std::string::npos);
        if (it % 3) CHECK(rec.find(q.substr(c.query_start - 5000000000ull, c.s.q_len)) != std::string::npos);
        ++sam;
      }
    }
  }
  printf("%ld CIGARs: %ld erosions, %ld start swaps, %ld end swaps, %ld independent tails held against a head patch, %ld later, %ld PAF and %ld SAM records\n", it,
         eroded, swaps_start, swaps_end, independent, later, paf, sam);
  return eroded && swaps_start && swaps_end && independent && later && paf && sam ? 0 : 2;
}
