// wfmash-hip -- command line front end of the MI355X build: map phase, align phase, or both, with
// the reference's flag names (src/interface/parse_args.hpp:61-138) for the options these phases read.
//
//   wfmash-hip target.fa [query.fa]            map, then align the mappings (PAF on stdout)
//   wfmash-hip -m target.fa [query.fa]         approximate mappings only (parse_args.hpp:77)
//   wfmash-hip -i map.paf target.fa [query.fa] align the mappings of a previous -m run (:119, :800-804)
//
//   wfmash-hip -W idx target.fa                build the target index, write it and stop (parse_args.hpp:745-751)
//   wfmash-hip -I idx target.fa [query.fa]     read the index instead of building it (:752-758)
//   wfmash-hip -K seeds.paf target.fa [query.fa]     external PAF seeds through the group sweep and the scaffold filter
//                                              in place of the MinHash mapper, then aligned (:78, :771-773); with -m the
//                                              filtered seeds are written (host only, no GPU is opened)
//   --scaffold-out FILE                        the scaffold chains the scaffold filter used as anchors (:105, :464-465),
//                                              of the map path or of -K
//   --streaming-minhash                        target sketches from one bottom-s MinHash per sequence instead of winnowed
//                                              minmers (:137, :177; winSketch.hpp:467-497); no effect with -K or -i
//   --resident-seqs                            whole sequences stay on the device (up to WFM_SEQSTORE_GB, 32) and the align phase names
//                                              its windows by reference instead of fetching and uploading each; off by default
//   --verify                                   every finished PAF line of the run is held against its bases on the device before it is
//                                              written (spans, run structure, every = and X base; not optimality); a failure is one line
//                                              on stderr and exit status 3 after everything has been written; refused together with -a
//   --verify-optimal [--verify-optimal-cells N] every score a device call of the align phase returns (main alignments, head and tail patches)
//                                              is proved optimal by a banded DP on the device (wfm_check_optimal); the output bytes do
//                                              not change; a failure is one line on stderr and exit status 3; N caps the DP cells of one
//                                              problem (problems beyond it are counted as skipped); allowed with --verify, -a and
//                                              --resident-seqs, refused with -m.  Costs far more than the alignment on near-identical records
//   --left-align                               every interior gap of the records' final CIGARs is moved to its leftmost placement on the
//                                              device before the record is written (wfm_left_align_runs: an indel in a homopolymer or a
//                                              tandem repeat lands where minimap2 and VCF normalisation put it); only cg:Z: changes in a
//                                              PAF line, only CIGAR and MD in a SAM record; allowed with -a, -d, --verify (which then checks
//                                              the normalised lines), --verify-optimal, --resident-seqs, --gpus, -i and -K, refused with -m;
//                                              off by default
//   --cs | --cs=short | --cs=long              minimap2's cs:Z: difference string as the last field of every PAF line and SAM record,
//                                              spelled on the device from the runs the record spells (wfm_cs_strings): which bases are
//                                              substituted, inserted and deleted (short), with the matching bases as well (long); the
//                                              value is attached with '=', so a following file name is never taken for it; nothing else
//                                              of a line changes; allowed with -a, -d, -i, -K, --gpus, --resident-seqs, --verify,
//                                              --verify-optimal and --left-align (the string is then that of the normalised runs),
//                                              refused with -m and --verify-paf; off by default
//   --variants FILE                            the substitutions, insertions and deletions of every record written, as a VCF: called on
//                                              the device from the runs the record spells, alleles included (wfm_call_variants); one line
//                                              per variant in PAF record order, ascending POS within a record, alleles on the target's
//                                              strand, INFO = QNAME, QSTART, QEND, QSTRAND; not sorted across records, no sample columns
//                                              (bcftools sort); no output byte of the PAF or SAM changes; allowed with -a, -d, -i, -K,
//                                              --gpus, --resident-seqs, --verify, --verify-optimal, --left-align (the variants are then
//                                              those of the normalised runs) and --cs, refused with -m and --verify-paf; off by default
//   --coverage FILE                            per-base depth of every target sequence as a bedGraph (name, start, end, depth; no track
//                                              line): depth = the number of records WRITTEN with an = or X base there (D bases do not
//                                              count), summed on the device over all batches and GPUs (wfm_coverage_*); sequences in index
//                                              order, maximal intervals of constant depth tiling [0, length), depth 0 included; 4 bytes of
//                                              device memory per target base on every handle (WFM_COV_GB, 32); no output byte of the PAF
//                                              or SAM changes; allowed with -a, -d, -i, -K, --gpus, --resident-seqs, --verify,
//                                              --verify-optimal, --left-align (the depth is then that of the normalised runs), --cs and
//                                              --variants, refused with -m and --verify-paf; off by default
//   --coverage-paf IN.paf --coverage FILE target.fa   the same file for an existing aligned PAF (this build's, the reference's,
//                                              minimap2 -c --eqx's): no mapping, no alignment; lines without an =XID cg:Z:, malformed
//                                              lines, unknown targets and other tlens are skipped and counted; only --device beside it
//   --lift IN.bed --lift-out FILE              where the BED's target intervals lie in every query: the intervals are lifted on the device
//                                              through the runs of every record WRITTEN (wfm_lift_runs; nothing goes up but runs), one
//                                              line per (record, overlapping interval) in the order of the PAF's records: qname qstart qend
//                                              name strand tname tstart tend istart iend eq x ins del; an interval in a deletion has
//                                              qstart == qend; no output byte of the PAF or SAM changes; allowed with -a, -d, -i, -K,
//                                              --gpus, --resident-seqs, --verify, --verify-optimal, --left-align (the lifts are then those
//                                              of the normalised runs), --cs, --variants and --coverage, refused with -m and --verify-paf;
//                                              each of the two is an error without the other; off by default
//   --lift-paf IN.paf --lift IN.bed --lift-out FILE target.fa   the same file for an existing aligned PAF: no mapping, no alignment;
//                                              lines are skipped and counted as --coverage-paf does; only --device beside it
//   --chain FILE [--chain-swap]                a UCSC chain file of every record WRITTEN, from the target to the query (what liftOver,
//                                              CrossMap and bcftools +liftover take): the runs are compacted to blocks and gaps on the device
//                                              (wfm_chain_runs; nothing goes up but runs), one chain per record in the order of the PAF's
//                                              records, ids 1, 2, 3 ... in file order; score = the record's = columns (it ranks chains, it is
//                                              not blastz's score); --chain-swap: the file chainSwap would make of it, from the query to the
//                                              target; no output byte of the PAF or SAM changes; allowed and refused beside what --lift is;
//                                              --chain-swap without --chain is an error; off by default
//   --chain-net FILE                           a single-coverage chain file: the blocks of every record WRITTEN go to a net object on the
//                                              device (wfm_net_*), which gives every target base to the record with the most = columns over
//                                              it (the earlier record where they are equal); once all are aligned, one chain per record that
//                                              won a base, from the pieces left to it, in the order of the PAF's records: an .over.chain for
//                                              liftOver, CrossMap and bcftools +liftover without chainSort | chainNet | netChainSubset; with
//                                              or without --chain, whose bytes do not change; refused where --chain is, and with
//                                              --chain-swap (nets on the query side are not done); off by default
//   --transitive IN.bed --transitive-out FILE [--transitive-depth N]   transitive lifts: the runs of every record WRITTEN go to a trans
//                                              object on the handle's device; after the last batch the BED's intervals are closed over all
//                                              records, both ways, N rounds deep (default 2, 0 = to the fixed point: include/wfmash_host.h)
//   --transitive-paf IN.paf --transitive IN.bed --transitive-out FILE [--transitive-depth N] target.fa [query.fa]   the same file for an
//                                              existing aligned PAF; nothing else runs
//   --chain-paf IN.paf [--chain FILE [--chain-swap]] [--chain-net FILE] target.fa [query.fa]   the same file(s) for an existing aligned
//                                              PAF, one of the two at least: no mapping, no alignment; lines are skipped and counted as
//                                              --coverage-paf does (the query's name and length are the line's: query.fa is not read);
//                                              only --device beside it
//   --maf FILE [--maf-split N]                 the aligned sequences of every record WRITTEN as pairwise MAF blocks (what multiz, PHAST,
//                                              mafTools and wgatools read; `wgatools paf2maf` makes it from a PAF with both FASTAs open
//                                              again): the two gapped rows are spelled on the device (wfm_maf_rows), one block per record,
//                                              or cut at every gap stretch of N or more gap bases (N as 5000, 10k; default 0 = never), whose
//                                              columns are then not written; "a score=" is the block's = columns; fields separated by single
//                                              spaces, not column-padded; in the order of the PAF's records; works with PAF and -a alike; no
//                                              output byte of the PAF or SAM changes; refused with -m and --verify-paf; --maf-split without
//                                              --maf is an error; off by default
//   --maf-paf IN.paf --maf FILE [--maf-split N] target.fa [query.fa]   the same file for an existing aligned PAF: no mapping, no
//                                              alignment; a line whose target target.fa does not have, or whose query query.fa (target.fa without it) does not
//                                              have, is skipped and counted; only --device
//                                              beside it
//   --pav IN.bed | --pav-window N, --pav-out FILE   which groups of query sequences (haplotypes, samples: the part of the name before its
//                                              last '#') have each target interval, and how much of it: the runs of every record WRITTEN go
//                                              into a per-group union of aligned segments on the device (wfm_pav_*; 16 bytes a segment, never
//                                              a dense array); one row per interval -- the BED's, or windows of N bases tiling every target
//                                              sequence -- and one column per group of the query FASTA, cells = bases of the interval under
//                                              an = or X base of at least one record of the group; the target's own group is a column like
//                                              the others (0 where the mapper skips self or same-group mappings); no output byte of the PAF
//                                              or SAM changes; refused with -m and --verify-paf; --pav and --pav-window exclude each other
//                                              and each needs --pav-out; off by default
//   --pav-paf IN.paf (--pav IN.bed | --pav-window N) --pav-out FILE target.fa [query.fa]   the same file for an existing aligned PAF: no
//                                              mapping, no alignment; lines are skipped and counted as --coverage-paf does, and a line whose
//                                              query is not in the query FASTA; only --device beside it
//   --genotypes FILE                           the variants of ALL records written merged into one VCF sorted by (sequence, POS, REF, ALT),
//                                              one line per distinct site and one haploid GT column per group of query sequences (--pav's
//                                              groups): 1 = a record of the group carries exactly this variant, 0 = the whole REF span lies
//                                              under = bases of the group's records, . = neither; AC and AN count the row.  The join (a
//                                              sort, a de-duplication on the allele bytes, the sites x groups table) runs on the device
//                                              (wfm_sites_*).  It does not imply --left-align: give both, or one indel in a repeat can be two
//                                              sites.  No output byte of the PAF, SAM or --variants file changes; refused with -m and
//                                              --verify-paf; off by default
//   --verify-paf FILE target.fa [query.fa]     the same check on an existing aligned PAF (this build's or the reference's): no mapping,
//                                              no alignment; exit status 3 if a line fails
//   --ani-matrix FILE [--ani-only]             the group-by-group ANI table the identity estimate (-p aniN) is made from, as TSV: per
//                                              (query group, target group) pair the sizes of the two pooled MinHash sketches, their shared
//                                              hashes (counted on the device, wfm_sketch_intersections), Jaccard and ANI; written before
//                                              mapping starts, also when -p gives a number, and the run then goes on unchanged (the reference
//                                              prints the table to stderr, map_stats.hpp:746-752).  --ani-only stops after the table: no
//                                              index, no PAF.  Refused with -i and with -K (no map phase)
//   --hg-filter n,D,conf                       numerator, ANI difference and confidence of the L1 / L2 cutoffs (:94, :700-725)
//   -B DIR / -Z                                directory of the map-to-align hand-off file [cwd] / keep that file (:134-135)
//   --quiet, --ani-sketch-size INT             accepted and without effect: there is no progress meter, and the identity
//                                              estimate's sketch size is 4096 in the reference too (map_stats.hpp:330)
//
// Differences: output goes to stdout or --out FILE; --device picks the GPU, --gpus N spreads the
// queries (map) and the mapping records (align) over N GPUs of the node.  -K together with -i, -W or
// -I is refused (the reference ignores the index flags there).  Options of the reference that belong
// to subsystems outside this build (wavefront plots -G/-u) are not accepted.
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <limits>
#include <regex>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wfmash_host.h"

static int64_t handy_parameter(const std::string& v) {  // utils.cpp:13-29 ("50k", "1m", "2g")
  if (v.empty()) return -1;
  double mult = 1;
  std::string t = v;
  const char c = t.back();
  if (c == 'k' || c == 'K') { mult = 1e3; t.pop_back(); }
  else if (c == 'm' || c == 'M') { mult = 1e6; t.pop_back(); }
  else if (c == 'g' || c == 'G') { mult = 1e9; t.pop_back(); }
  if (t.empty() || t.find_first_not_of("0123456789.") != std::string::npos) return -1;
  return (int64_t)(atof(t.c_str()) * mult);
}

// --hg-filter n,D,conf (parse_args.hpp:700-725): false with the message printed when the value is refused
static bool parse_hg_filter(const std::string& v, wfmh_map_params_t* mp) {
  std::vector<std::string> params;  // CommonFunc::split: std::getline on ',' (commonFunc.hpp:744-757)
  std::stringstream ss(v);
  for (std::string item; std::getline(ss, item, ',');) params.push_back(item);
  if (params.size() != 3) {
    fprintf(stderr, "[wfmash] ERROR: hypergeometric filter requires 3 comma-separated values: numerator,ani-diff,confidence\n");
    return false;
  }
  double x[3];
  for (int j = 0; j < 3; ++j) {  // std::stod: a number at the start of the value, or it throws
    const char* c = params[(size_t)j].c_str();
    char* end = nullptr;
    x[j] = strtod(c, &end);
    if (end == c) { fprintf(stderr, "[wfmash] ERROR: --hg-filter expects numbers, got: %s\n", c); return false; }
    if (j == 0 && x[0] < 1.0) { fprintf(stderr, "[wfmash] ERROR: hg-filter numerator must be >= 1.0\n"); return false; }
  }
  mp->hg_numerator = x[0];
  mp->ani_diff = (float)(x[1] / 100.0);
  mp->ani_diff_conf = (float)(x[2] / 100.0);
  return true;
}

static void usage() {
  fprintf(stderr,
          "usage: wfmash-hip [options] target.fa [query.fa]\n"
          "  phases    -m approximate mappings only | -i FILE align mappings from FILE | (neither) map + align\n"
          "  mapping   -p PCT|aniN[+-X] identity [ani50-2]   -k INT k-mer [15]   -w INT window [1k]   -s INT sketch size [auto]\n"
          "            -n INT|inf mappings per segment [inf]   -l INT block length [0]   -c INT chain jump [2k]   -P INT|inf max length [50k]\n"
          "            -N no split   -M no merge   -f no filter   -o one-to-one   -O FLOAT max overlap [0.95]   -x FLOAT sparsify [1.0]\n"
          "            -H INT L1 hits [3]   -F FLOAT high-frequency filter [0.0002]   -b SIZE target batch [all]\n"
          "            --hg-filter n,D,conf hypergeometric filter [1.0,0.0,99.9]   --ani-sketch-size INT (no effect)\n"
          "            --ani-matrix FILE write the group-by-group ANI table the identity estimate is made from (TSV), then go on\n"
          "            --ani-only stop after the table (needs --ani-matrix)\n"
          "            -W FILE build the index, write it and stop   -I FILE read the index from FILE\n"
          "            --streaming-minhash target sketches from a per-sequence bottom-s MinHash (experimental)\n"
          "            -K FILE external PAF seeds in place of the mapper ('-' = stdin)\n"
          "            -S INT scaffold mass [10k]   -D INT scaffold dist [100k]   -j INT scaffold jump [100k]   -r INT per scaffold [1]\n"
          "            --scaffold-out FILE write the scaffold chains\n"
          "            -Y C group delimiter [#]   -X self maps   -L lower triangular   -t INT threads [1]\n"
          "  alignment -g x,o1,e1,o2,e2 [5,8,2,24,1]   -E INT target padding   -U INT query padding   -a SAM   -d MD tag\n"
          "            --resident-seqs keep whole sequences on the GPU and align windows of them by reference [off]\n"
          "            --verify check every PAF line written against its bases on the GPU (exit status 3 if one fails; not with -a)\n"
          "            --verify-optimal prove every alignment score optimal by a banded DP on the GPU (slow; exit status 3 if one is not; not with -m)\n"
          "            --verify-optimal-cells N skip problems whose band holds more than N DP cells [no cap]\n"
          "            --left-align move every interior gap of the final CIGARs to its leftmost placement on the GPU (only cg:Z: / CIGAR and MD change; not with -m)\n"
          "            --cs[=short|=long] append minimap2's cs:Z: difference string, spelled on the GPU, to every PAF line / SAM record (not with -m, --verify-paf)\n"
          "            --variants FILE write the SNVs, insertions and deletions of every record, called on the GPU, as a VCF (unsorted; not with -m, --verify-paf)\n"
          "            --coverage FILE write the per-base depth of every target sequence, summed on the GPU over the records written, as a bedGraph (not with -m, --verify-paf)\n"
          "            --coverage-paf FILE with --coverage: the depth of an existing aligned PAF over target.fa, and stop (only --device beside it)\n"
          "            --lift BED --lift-out FILE lift the BED's target intervals through every record written, on the GPU: one line per record and interval (not with -m, --verify-paf)\n"
          "            --lift-paf FILE with --lift, --lift-out: lift through an existing aligned PAF over target.fa, and stop (only --device beside it)\n"
          "            --chain FILE  write a UCSC chain file (target to query) of every record written, blocks and gaps made on the GPU; score = the = columns (not with -m, --verify-paf)\n"
          "            --maf FILE    write the aligned sequences of every record as pairwise MAF blocks, rows spelled on the GPU (single spaces, no column padding; not with -m, --verify-paf)\n"
          "            --maf-split N with --maf: end a block at every gap stretch of N or more gap bases (5000, 10k; default 0 = one block per record)\n"
          "            --maf-paf FILE with --maf: the MAF file of an existing aligned PAF over target.fa [query.fa], and stop (only --maf-split and --device beside it)\n"
          "            --chain-swap  with --chain: the swapped file (query to target), what chainSwap would make of it\n"
          "            --chain-net FILE write a single-coverage chain file: every target base under at most one chain, the best record's, from a net across the records on the GPU (with or without --chain; not with -m, --verify-paf, --chain-swap)\n"
          "            --transitive IN.bed --transitive-out FILE [--transitive-depth N]  close the BED's intervals over ALL records written, through targets and queries alike, on the GPU: every interval a seed reaches in N rounds (2; 0: to the fixed point) as 'seq start end name seed_seq seed_start seed_end' (not with -m, --verify-paf)\n"
          "            --transitive-paf FILE with --transitive and --transitive-out: the same file for an existing aligned PAF over target.fa [query.fa], and stop (only --transitive-depth and --device beside it)\n"
          "            --chain-paf FILE with --chain and/or --chain-net: the chain file(s) of an existing aligned PAF over target.fa, and stop (only --chain-swap and --device beside it)\n"
          "            --pav BED | --pav-window N, --pav-out FILE per target interval and group of query sequences the bases present, from per-group unions on the GPU (not with -m, --verify-paf)\n"
          "            --genotypes FILE write ONE sorted VCF of the distinct variants of all records with a haploid GT column (0, 1, .) per group of query sequences, joined on the GPU (give --left-align too; not with -m, --verify-paf)\n"
          "            --pav-paf FILE with --pav or --pav-window, --pav-out: the table of an existing aligned PAF over target.fa [query.fa], and stop (only --device beside it)\n"
          "            --verify-paf FILE check an existing aligned PAF against target.fa [query.fa] and stop (exit status 3 if a line fails)\n"
          "  other     --out FILE [stdout]   --device INT [0]   --gpus N|all [1] GPUs of this node, starting at --device\n"
          "            -B DIR directory of the hand-off file [cwd]   -Z keep the hand-off file   --quiet (no effect)\n");
}

// A mode that works on an existing PAF and runs nothing else: a handle on the device for call(h) -> WFM_*, the handle's message under the
// mode's tag where that fails.  The exit status: 0, `failed`, or 2 without a device.
template <class Call>
static int offline_mode(int device, const char* tag, Call call, int failed = 2) {
  wfm_handle_t* h = nullptr;
  if (wfm_create(device, &h) != WFM_OK) { fprintf(stderr, "[wfmash] ERROR: no usable MI355X device %d (there is no CPU fallback)\n", device); return 2; }
  const int rc = call(h);
  if (rc != WFM_OK) fprintf(stderr, "[wfmash::%s] ERROR: %s\n", tag, wfm_last_error(h));
  wfm_destroy(h);
  return rc == WFM_OK ? 0 : failed;
}

int main(int argc, char** argv) {
  wfmh_align_params_t ap;
  wfmh_align_default_params(&ap);
  ap.threads = 1;  // -t, default 1 as in the reference (parse_args.hpp: thread_count); the C ABI default (0) means all cores
  wfmh_map_params_t mp;
  wfmh_map_default_params(&mp);
  std::string mapping_in, out = "/dev/stdout", target, query, seeds_in, scaffold_out, tmp_base, verify_in, ani_matrix_out, variants_out, genotypes_out, coverage_out, coverage_in, lift_bed, lift_out, lift_in, pav_bed, pav_out, pav_in, chain_out, chain_in, chain_net_out, trans_bed, trans_out, trans_in, maf_out, maf_in;
  unsigned long trans_depth = 2;
  uint64_t pav_window = 0;
  bool pav_window_set = false;
  bool pav_other = false;      // --pav-paf: anything beside it, --pav, --pav-window, --pav-out, --device and the two FASTAs
  bool other_options = false;  // --coverage-paf: anything beside it, --coverage, --device and the target
  bool lift_other = false;     // --lift-paf: anything beside it, --lift, --lift-out, --device and the target
  bool chain_other = false;    // --chain-paf: anything beside it, --chain, --chain-swap, --device and the two FASTAs
  bool trans_other = false;    // --transitive-paf: anything beside it, --transitive, --transitive-out, --transitive-depth, --device and the two FASTAs
  bool chain_swap = false;
  bool maf_other = false;      // --maf-paf: anything beside it, --maf, --maf-split, --device and the two FASTAs
  int64_t maf_split = -1;      // --maf-split: -1 not given
  bool verify = false, verify_optimal = false, ani_only = false, left_align = false;
  uint64_t verify_optimal_cells = 0;
  int cs_form = 0;  // --cs: 0 off, 1 short, 2 long
  bool approx_only = false, target_padding_given = false, query_padding_given = false, keep_temp = false;
  int device = 0, gpus = 1;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a[0] == '-' ? (a != "--pav" && a != "--pav-window" && a != "--pav-out" && a != "--pav-paf" && a != "--device" && a != "-h" && a != "--help") : !query.empty()) pav_other = true;
    if (a[0] == '-' ? (a != "--transitive" && a != "--transitive-out" && a != "--transitive-depth" && a != "--transitive-paf" && a != "--device" && a != "-h" && a != "--help") : !query.empty()) trans_other = true;
    if (a[0] == '-' ? (a != "--chain" && a != "--chain-net" && a != "--chain-swap" && a != "--chain-paf" && a != "--device" && a != "-h" && a != "--help") : !query.empty()) chain_other = true;
    if (a[0] == '-' ? (a != "--maf" && a != "--maf-split" && a != "--maf-paf" && a != "--device" && a != "-h" && a != "--help") : !query.empty()) maf_other = true;
    if (a[0] == '-' ? (a != "--lift" && a != "--lift-out" && a != "--lift-paf" && a != "--device" && a != "-h" && a != "--help") : !target.empty()) lift_other = true;
    if (a[0] == '-' ? (a != "--coverage" && a != "--coverage-paf" && a != "--device" && a != "-h" && a != "--help") : !target.empty()) other_options = true;
    auto next = [&](const char* name) -> std::string {
      if (i + 1 >= argc) { fprintf(stderr, "[wfmash] ERROR: missing value for %s\n", name); exit(1); }
      return argv[++i];
    };
    auto size = [&](const char* name) -> int64_t {
      const int64_t v = handy_parameter(next(name));
      if (v < 0) { fprintf(stderr, "[wfmash] ERROR: %s expects a size such as 5000, 50k, 1m\n", name); exit(1); }
      return v;
    };
    if (a == "-m" || a == "--approx-mapping") approx_only = true;
    else if (a == "-i" || a == "--align-paf") mapping_in = next("-i");
    else if (a == "-K" || a == "--input-seeds") seeds_in = next("-K");
    else if (a == "--scaffold-out") { scaffold_out = next("--scaffold-out"); mp.scaffold_out = scaffold_out.c_str(); }
    else if (a == "--out") out = next("--out");
    else if (a == "--device") device = atoi(next("--device").c_str());
    else if (a == "--gpus") { const std::string v = next("--gpus"); gpus = v == "all" ? 0 : atoi(v.c_str()); if (gpus < 0) gpus = 1; }
    else if (a == "-t" || a == "--threads") { mp.threads = atoi(next("-t").c_str()); ap.threads = mp.threads; }
    // ---- system (parse_args.hpp:134-137)
    else if (a == "-B" || a == "--tmp-base") tmp_base = next("-B");
    else if (a == "-Z" || a == "--keep-temp") keep_temp = true;
    else if (a == "--quiet") {}  // no progress meter to turn off
    else if (a == "--streaming-minhash") mp.streaming_minhash = 1;
    else if (a == "--ani-matrix") ani_matrix_out = next("--ani-matrix");
    else if (a == "--ani-only") ani_only = true;
    // ---- mapping (parse_args.hpp:71-115)
    else if (a == "-k" || a == "--kmer-size") mp.kmer_size = atoi(next("-k").c_str());
    else if (a == "-s" || a == "--sketch-size") mp.sketch_size = atoi(next("-s").c_str());
    else if (a == "-w" || a == "--window-size") {
      mp.window_length = size("-w");
      if (mp.window_length <= 0) { fprintf(stderr, "[wfmash] ERROR, skch::parseandSave, window size has to be a float value greater than 0.\n"); return 1; }
      if (mp.window_length < 100) {  // parse_args.hpp:324-328
        fprintf(stderr, "[wfmash] ERROR, skch::parseandSave, minimum window size is required to be >= 100 bp.\n");
        return 1;
      }
    }
    else if (a == "-p" || a == "--map-pct-id") {
      const std::string v = next("-p");
      std::smatch m;
      if (std::regex_match(v, m, std::regex("^ani(\\d+)([+-]\\d+)?$"))) {  // parse_args.hpp:345-366
        mp.auto_pct_identity = 1;
        mp.ani_percentile = atoi(m[1].str().c_str());
        if (mp.ani_percentile < 1 || mp.ani_percentile > 99) {  // :352-356
          fprintf(stderr, "[wfmash] ERROR: ANI percentile must be between 1 and 99, got: %d\n", mp.ani_percentile);
          return 1;
        }
        mp.ani_adjustment = m[2].matched ? (float)atof(m[2].str().c_str()) : 0.0f;
      } else if (v == "auto") {
        mp.auto_pct_identity = 1; mp.ani_percentile = 25; mp.ani_adjustment = 0.0f;
      } else {
        char* end = nullptr;
        const float pct = strtof(v.c_str(), &end);
        if (end == v.c_str()) {  // std::stof throws (:383-387)
          fprintf(stderr, "[wfmash] ERROR: Invalid value for -p/--map-pct-id: %s\n", v.c_str());
          return 1;
        }
        if (pct < 50) {  // :377-380
          fprintf(stderr, "[wfmash] ERROR: minimum nucleotide identity requirement should be >= 50%%.\n");
          return 1;
        }
        mp.auto_pct_identity = 0;
        mp.percentage_identity = pct / 100.0f;
      }
    }
    else if (a == "-n" || a == "--mappings") {
      const std::string v = next("-n");
      mp.num_mappings_for_segment = (v == "inf" || v == "-1") ? std::numeric_limits<uint32_t>::max() : (uint32_t)atoll(v.c_str());
    }
    else if (a == "-l" || a == "--block-length") mp.block_length = size("-l");
    else if (a == "-c" || a == "--chain-jump") mp.chain_gap = size("-c");
    else if (a == "-P" || a == "--max-length") {  // parse_args.hpp:472-483: "inf" = no limit
      if (i + 1 < argc && std::string(argv[i + 1]) == "inf") { ++i; mp.max_mapping_length = (uint64_t)std::numeric_limits<int64_t>::max(); }
      else mp.max_mapping_length = (uint64_t)size("-P");
      if (mp.max_mapping_length == 0) { fprintf(stderr, "[wfmash] ERROR: max mapping length must be greater than 0.\n"); return 1; }
    }
    else if (a == "-N" || a == "--no-split") mp.split = 0;
    else if (a == "-M" || a == "--no-merge") mp.merge_mappings = 0;
    else if (a == "-f" || a == "--no-filter") mp.filter_mode = 3;
    else if (a == "-o" || a == "--one-to-one") mp.filter_mode = 2;
    else if (a == "-O" || a == "--overlap") mp.overlap_threshold = atof(next("-O").c_str());
    else if (a == "-x" || a == "--sparsify") {
      const double f = atof(next("-x").c_str());
      mp.sparsity_hash_threshold = f == 1 ? std::numeric_limits<uint64_t>::max() : (uint64_t)(f * (double)std::numeric_limits<uint64_t>::max());
    }
    else if (a == "-H" || a == "--l1-hits") mp.minimum_hits = atoi(next("-H").c_str());
    else if (a == "--hg-filter") { if (!parse_hg_filter(next("--hg-filter"), &mp)) return 1; }
    else if (a == "--ani-sketch-size") {  // stored by the reference, never read: the estimate's sketch is 4096 (map_stats.hpp:330)
      const std::string v = next("--ani-sketch-size");
      char* end = nullptr;
      (void)strtol(v.c_str(), &end, 10);
      if (v.empty() || *end) { fprintf(stderr, "[wfmash] ERROR: --ani-sketch-size expects an integer, got: %s\n", v.c_str()); return 1; }
    }
    else if (a == "-F" || a == "--filter-freq") mp.max_kmer_freq = atof(next("-F").c_str());
    else if (a == "-b" || a == "--batch") mp.index_by_size = size("-b");
    else if (a == "-W" || a == "--write-index") { mp.index_file = argv[(next("-W"), i)]; mp.write_index = 1; }
    else if (a == "-I" || a == "--read-index") { mp.index_file = argv[(next("-I"), i)]; mp.write_index = 0; }
    else if (a == "-S" || a == "--scaffold-mass") mp.scaffold_min_length = size("-S");
    else if (a == "-D" || a == "--scaffold-dist") mp.scaffold_max_deviation = size("-D");
    else if (a == "-j" || a == "--scaffold-jump") mp.scaffold_gap = size("-j");
    else if (a == "-r" || a == "--retain-per-scaffold") {
      const std::string v = next("-r");
      mp.num_mappings_for_scaffold = (v == "inf" || v == "-1") ? std::numeric_limits<uint32_t>::max() : (uint32_t)atoll(v.c_str());
    }
    else if (a == "--scaffold-overlap") mp.scaffold_overlap_threshold = atof(next("--scaffold-overlap").c_str());
    else if (a == "-Y" || a == "--group-prefix") { const std::string v = next("-Y"); mp.prefix_delim = v.empty() ? '\0' : v[0]; mp.skip_prefix = mp.prefix_delim != '\0'; }
    else if (a == "-T" || a == "--target-prefix") mp.target_prefix = argv[(next("-T"), i)];
    else if (a == "-R" || a == "--target-list") mp.target_list = argv[(next("-R"), i)];
    else if (a == "-Q" || a == "--query-prefix") mp.query_prefix = argv[(next("-Q"), i)];
    else if (a == "-A" || a == "--query-list") mp.query_list = argv[(next("-A"), i)];
    else if (a == "-X" || a == "--self-maps") mp.skip_self = 0;
    else if (a == "-L" || a == "--lower-triangular") mp.lower_triangular = 1;
    // ---- alignment (parse_args.hpp:119-129)
    else if (a == "-E" || a == "--target-padding") { ap.target_padding = (uint64_t)size("-E"); target_padding_given = true; }
    else if (a == "-U" || a == "--query-padding") { ap.query_padding = (uint64_t)size("-U"); query_padding_given = true; }
    else if (a == "-g" || a == "--wfa-params") {
      const std::string v = next("-g");
      if (sscanf(v.c_str(), "%d,%d,%d,%d,%d", &ap.mismatch, &ap.gap_open1, &ap.gap_ext1, &ap.gap_open2, &ap.gap_ext2) != 5) {
        fprintf(stderr, "[wfmash] ERROR: --wfa-params expects 5 values\n");
        return 1;
      }
    }
    else if (a == "--min-length") ap.min_alignment_length = (uint64_t)atoll(next("--min-length").c_str());
    else if (a == "--min-block-id") ap.min_block_identity = (float)atof(next("--min-block-id").c_str());
    else if (a == "--no-patching") ap.disable_chain_patching = 1;
    else if (a == "-a" || a == "--sam") ap.sam_format = 1;
    else if (a == "-d" || a == "--md-tag") ap.emit_md_tag = 1;
    else if (a == "--resident-seqs") ap.resident_sequences = 1;
    else if (a == "--verify") verify = true;
    else if (a == "--verify-optimal") verify_optimal = true;
    else if (a == "--left-align") left_align = true;
    else if (a == "--cs" || a == "--cs=short") cs_form = 1;
    else if (a == "--cs=long") cs_form = 2;
    else if (a.compare(0, 5, "--cs=") == 0) { fprintf(stderr, "[wfmash] ERROR: --cs takes =short or =long, not '%s'\n", a.c_str() + 5); return 1; }
    else if (a == "--variants") variants_out = next("--variants");
    else if (a == "--genotypes") genotypes_out = next("--genotypes");
    else if (a == "--coverage") coverage_out = next("--coverage");
    else if (a == "--coverage-paf") coverage_in = next("--coverage-paf");
    else if (a == "--lift") lift_bed = next("--lift");
    else if (a == "--lift-out") lift_out = next("--lift-out");
    else if (a == "--lift-paf") lift_in = next("--lift-paf");
    else if (a == "--chain") chain_out = next("--chain");
    else if (a == "--chain-net") chain_net_out = next("--chain-net");
    else if (a == "--transitive") trans_bed = next("--transitive");
    else if (a == "--transitive-out") trans_out = next("--transitive-out");
    else if (a == "--transitive-paf") trans_in = next("--transitive-paf");
    else if (a == "--transitive-depth") {
      const std::string v = next("--transitive-depth");
      char* end = nullptr;
      trans_depth = strtoul(v.c_str(), &end, 10);
      if (v.empty() || *end || v[0] == '-' || trans_depth > 0xfffffffful) { fprintf(stderr, "[wfmash] ERROR: --transitive-depth takes a number of rounds, 0 for the fixed point\n"); return 1; }
    }
    else if (a == "--chain-swap") chain_swap = true;
    else if (a == "--maf") maf_out = next("--maf");
    else if (a == "--maf-split") maf_split = size("--maf-split");
    else if (a == "--maf-paf") maf_in = next("--maf-paf");
    else if (a == "--chain-paf") chain_in = next("--chain-paf");
    else if (a == "--pav") pav_bed = next("--pav");
    else if (a == "--pav-out") pav_out = next("--pav-out");
    else if (a == "--pav-paf") pav_in = next("--pav-paf");
    else if (a == "--pav-window") {
      const std::string v = next("--pav-window");
      char* end = nullptr;
      pav_window = std::strtoull(v.c_str(), &end, 10);
      if (v.empty() || *end || v[0] == '-' || pav_window == 0) { fprintf(stderr, "[wfmash] ERROR: --pav-window takes a positive number of bases\n"); return 1; }
      pav_window_set = true;
    }
    else if (a == "--verify-optimal-cells") verify_optimal_cells = std::strtoull(next("--verify-optimal-cells").c_str(), nullptr, 10);
    else if (a == "--verify-paf") verify_in = next("--verify-paf");
    else if (a == "-h" || a == "--help") { usage(); return 0; }
    else if (a == "-v" || a == "--version") { std::printf("%s\n", WFMASH_HIP_VERSION); return 0; }
    else if (a[0] != '-') { if (target.empty()) target = a; else query = a; }
    else { fprintf(stderr, "[wfmash] unknown option %s\n", a.c_str()); usage(); return 1; }
  }
  if (target.empty()) { fprintf(stderr, "[wfmash] ERROR: need a target FASTA\n"); usage(); return 1; }
  if (verify && ap.sam_format) { fprintf(stderr, "[wfmash] ERROR: --verify reads the =/X CIGAR of PAF lines: it cannot be combined with -a (SAM)\n"); return 1; }
  if (verify && approx_only) { fprintf(stderr, "[wfmash] ERROR: --verify checks alignments: it cannot be combined with -m\n"); return 1; }
  if (left_align && approx_only) { fprintf(stderr, "[wfmash] ERROR: --left-align normalises alignments: it cannot be combined with -m\n"); return 1; }
  if (cs_form && approx_only) { fprintf(stderr, "[wfmash] ERROR: --cs spells alignments: it cannot be combined with -m\n"); return 1; }
  if (cs_form && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --cs belongs to the align phase: it cannot be combined with --verify-paf\n"); return 1; }
  if (!variants_out.empty() && approx_only) { fprintf(stderr, "[wfmash] ERROR: --variants calls alignments: it cannot be combined with -m\n"); return 1; }
  if (!variants_out.empty() && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --variants belongs to the align phase: it cannot be combined with --verify-paf\n"); return 1; }
  if (!coverage_out.empty() && approx_only) { fprintf(stderr, "[wfmash] ERROR: --coverage counts alignments: it cannot be combined with -m\n"); return 1; }
  if (!coverage_out.empty() && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --coverage belongs to the align phase: it cannot be combined with --verify-paf\n"); return 1; }
  if (!coverage_in.empty() && coverage_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --coverage-paf needs --coverage FILE\n"); return 1; }
  if (!lift_bed.empty() && lift_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --lift needs --lift-out FILE\n"); return 1; }
  if (lift_bed.empty() && !lift_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --lift-out needs --lift IN.bed\n"); return 1; }
  if (!lift_in.empty() && lift_bed.empty()) { fprintf(stderr, "[wfmash] ERROR: --lift-paf needs --lift IN.bed and --lift-out FILE\n"); return 1; }
  if (!lift_bed.empty() && approx_only) { fprintf(stderr, "[wfmash] ERROR: --lift lifts through alignments: it cannot be combined with -m\n"); return 1; }
  if (!lift_bed.empty() && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --lift belongs to the align phase: it cannot be combined with --verify-paf\n"); return 1; }
  if (!genotypes_out.empty() && approx_only) { fprintf(stderr, "[wfmash] ERROR: --genotypes reads alignments: it cannot be combined with -m\n"); return 1; }
  if (!genotypes_out.empty() && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --genotypes belongs to the align phase: it cannot be combined with --verify-paf\n"); return 1; }
  if (!trans_bed.empty() && trans_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --transitive needs --transitive-out FILE\n"); return 1; }
  if (trans_bed.empty() && !trans_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --transitive-out needs --transitive IN.bed\n"); return 1; }
  if (!trans_in.empty() && trans_bed.empty()) { fprintf(stderr, "[wfmash] ERROR: --transitive-paf needs --transitive IN.bed and --transitive-out FILE\n"); return 1; }
  if (!trans_in.empty() && trans_other) { fprintf(stderr, "[wfmash] ERROR: --transitive-paf runs nothing else: besides --transitive IN.bed, --transitive-out FILE, --transitive-depth N and the FASTAs it takes the number of the GPU only\n"); return 1; }
  if (!trans_bed.empty() && approx_only) { fprintf(stderr, "[wfmash] ERROR: --transitive lifts through alignments: it cannot be combined with -m\n"); return 1; }
  if (!trans_bed.empty() && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --transitive belongs to the align phase: it cannot be combined with --verify-paf\n"); return 1; }
  if (maf_split >= 0 && maf_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --maf-split needs --maf FILE\n"); return 1; }
  if (maf_split > 0xffffffffll) { fprintf(stderr, "[wfmash] ERROR: --maf-split expects a number of gap bases below 2^32\n"); return 1; }
  if (!maf_in.empty() && maf_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --maf-paf needs --maf FILE\n"); return 1; }
  if (!maf_out.empty() && approx_only) { fprintf(stderr, "[wfmash] ERROR: --maf spells alignments: it cannot be combined with -m\n"); return 1; }
  if (!maf_out.empty() && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --maf belongs to the align phase: it cannot be combined with --verify-paf\n"); return 1; }
  if (!maf_in.empty() && maf_other) { fprintf(stderr, "[wfmash] ERROR: --maf-paf runs nothing else: besides --maf FILE, --maf-split N and the FASTAs it takes the number of the GPU only\n"); return 1; }
  if (!chain_net_out.empty() && chain_swap) { fprintf(stderr, "[wfmash] ERROR: --chain-net cannot be combined with --chain-swap: nets on the query side are not done\n"); return 1; }
  if (chain_swap && chain_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --chain-swap needs --chain FILE\n"); return 1; }
  if (!chain_in.empty() && chain_out.empty() && chain_net_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --chain-paf needs --chain FILE\n"); return 1; }
  if (!chain_net_out.empty() && approx_only) { fprintf(stderr, "[wfmash] ERROR: --chain-net writes chains of alignments: it cannot be combined with -m\n"); return 1; }
  if (!chain_net_out.empty() && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --chain-net belongs to the align phase: it cannot be combined with --verify-paf\n"); return 1; }
  if (!chain_out.empty() && approx_only) { fprintf(stderr, "[wfmash] ERROR: --chain writes chains of alignments: it cannot be combined with -m\n"); return 1; }
  if (!chain_out.empty() && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --chain belongs to the align phase: it cannot be combined with --verify-paf\n"); return 1; }
  if (!chain_in.empty() && chain_other) { fprintf(stderr, "[wfmash] ERROR: --chain-paf runs nothing else: besides --chain FILE, --chain-swap and the FASTAs it takes the number of the GPU only\n"); return 1; }
  if (!lift_in.empty() && lift_other) { fprintf(stderr, "[wfmash] ERROR: --lift-paf runs nothing else: besides --lift IN.bed, --lift-out FILE and the target FASTA it takes the number of the GPU only\n"); return 1; }
  const bool pav_on = !pav_bed.empty() || pav_window_set;
  if (!pav_bed.empty() && pav_window_set) { fprintf(stderr, "[wfmash] ERROR: --pav IN.bed and --pav-window N exclude each other\n"); return 1; }
  if (pav_on && pav_out.empty()) { fprintf(stderr, "[wfmash] ERROR: %s needs --pav-out FILE\n", pav_window_set ? "--pav-window" : "--pav"); return 1; }
  if (!pav_on && !pav_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --pav-out needs --pav IN.bed or --pav-window N\n"); return 1; }
  if (!pav_in.empty() && !pav_on) { fprintf(stderr, "[wfmash] ERROR: --pav-paf needs --pav IN.bed or --pav-window N, and --pav-out FILE\n"); return 1; }
  if (pav_on && approx_only) { fprintf(stderr, "[wfmash] ERROR: --pav reads alignments: it cannot be combined with -m\n"); return 1; }
  if (pav_on && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --pav belongs to the align phase: it cannot be combined with --verify-paf\n"); return 1; }
  if (!pav_in.empty() && pav_other) { fprintf(stderr, "[wfmash] ERROR: --pav-paf runs nothing else: besides --pav IN.bed or --pav-window N, --pav-out FILE and the FASTAs it takes the number of the GPU only\n"); return 1; }
  if (!coverage_in.empty() && other_options) { fprintf(stderr, "[wfmash] ERROR: --coverage-paf runs nothing else: besides --coverage FILE and the target FASTA it takes the number of the GPU only\n"); return 1; }
  if (verify_optimal && approx_only) { fprintf(stderr, "[wfmash] ERROR: --verify-optimal checks alignment scores: it cannot be combined with -m\n"); return 1; }
  if (verify_optimal_cells && !verify_optimal) { fprintf(stderr, "[wfmash] ERROR: --verify-optimal-cells needs --verify-optimal\n"); return 1; }
  if (ani_only && ani_matrix_out.empty()) { fprintf(stderr, "[wfmash] ERROR: --ani-only needs --ani-matrix FILE\n"); return 1; }
  if (!ani_matrix_out.empty() && !mapping_in.empty()) {
    fprintf(stderr, "[wfmash] ERROR: --ani-matrix belongs to the map phase: it cannot be combined with -i (align mappings from a file)\n");
    return 1;
  }
  if (!ani_matrix_out.empty() && !seeds_in.empty()) {
    fprintf(stderr, "[wfmash] ERROR: --ani-matrix belongs to the map phase: it cannot be combined with -K (external seeds)\n");
    return 1;
  }
  if (!ani_matrix_out.empty() && !verify_in.empty()) { fprintf(stderr, "[wfmash] ERROR: --ani-matrix cannot be combined with --verify-paf\n"); return 1; }
  const char* const query_or_null = query.empty() ? nullptr : query.c_str();
  uint64_t oc[4] = {0, 0, 0, 0};  // (what a mode counted: only --verify-paf reads it)
  if (!pav_in.empty())  // the presence table of an existing PAF; nothing else runs
    return offline_mode(device, "pav", [&](wfm_handle_t* h) {
      return wfmh_pav_paf(h, target.c_str(), query_or_null, pav_in.c_str(), pav_bed.empty() ? nullptr : pav_bed.c_str(), pav_window, pav_out.c_str(), oc);
    });
  if (!maf_in.empty())  // the MAF file of an existing PAF; nothing else runs
    return offline_mode(device, "maf", [&](wfm_handle_t* h) {
      return wfmh_maf_paf(h, target.c_str(), query_or_null, maf_in.c_str(), maf_out.c_str(), (uint32_t)std::max<int64_t>(0, maf_split), oc);
    });
  if (!chain_in.empty())  // the chain file of an existing PAF; nothing else runs
    return offline_mode(device, "chain", [&](wfm_handle_t* h) {
      const int rc = chain_out.empty() ? WFM_OK : wfmh_chain_paf(h, target.c_str(), chain_in.c_str(), chain_out.c_str(), chain_swap ? 1 : 0, oc);
      return rc == WFM_OK && !chain_net_out.empty() ? wfmh_chain_net_paf(h, target.c_str(), chain_in.c_str(), chain_net_out.c_str(), oc) : rc;
    });
  if (!trans_in.empty())  // the seeds closed over an existing PAF; nothing else runs
    return offline_mode(device, "transitive", [&](wfm_handle_t* h) {
      return wfmh_transitive_paf(h, target.c_str(), query_or_null, trans_in.c_str(), trans_bed.c_str(), trans_out.c_str(), (uint32_t)trans_depth, oc);
    });
  if (!lift_in.empty())  // the BED through an existing PAF; nothing else runs
    return offline_mode(device, "lift", [&](wfm_handle_t* h) { return wfmh_lift_paf(h, target.c_str(), lift_in.c_str(), lift_bed.c_str(), lift_out.c_str(), oc); });
  if (!coverage_in.empty())  // the depth of an existing PAF; nothing else runs
    return offline_mode(device, "coverage", [&](wfm_handle_t* h) { return wfmh_coverage_paf(h, target.c_str(), coverage_in.c_str(), coverage_out.c_str(), oc); });
  if (!verify_in.empty()) {  // an existing PAF against its sequences; nothing else runs: 3 if a line failed or the check could not run
    const int code = offline_mode(device, "verify", [&](wfm_handle_t* h) {
      const int rc = wfmh_verify_paf(h, target.c_str(), query_or_null, verify_in.c_str(), oc);
      if (rc == WFM_OK)
        fprintf(stderr, "[wfmash::verify] %llu lines checked, %llu failed, %llu unverifiable, %llu bases compared\n", (unsigned long long)oc[0], (unsigned long long)oc[1],
                (unsigned long long)oc[2], (unsigned long long)oc[3]);
      return rc;
    }, 3);
    return code == 0 && oc[1] != 0 ? 3 : code;
  }
  if (approx_only && !mapping_in.empty()) { fprintf(stderr, "[wfmash] ERROR: -m and -i exclude each other\n"); return 1; }
  if (!seeds_in.empty() && !mapping_in.empty()) { fprintf(stderr, "[wfmash] ERROR: -K (external seeds) and -i (align mappings from a file) exclude each other\n"); return 1; }
  if (!seeds_in.empty() && mp.index_file) { fprintf(stderr, "[wfmash] ERROR: -K (external seeds) does not read or write an index (-W / -I)\n"); return 1; }
  if (!mapping_in.empty() && mp.index_file) { fprintf(stderr, "[wfmash] ERROR: -i (align only) does not read or write an index (-W / -I)\n"); return 1; }
  if (!approx_only && !(mp.index_file && mp.write_index) && mp.window_length > 10000) {  // parse_args.hpp:330-335
    fprintf(stderr, "[wfmash] ERROR: window size (-w) must be <= 10kb when running alignment.\n"
                    "[wfmash] For larger values, use -m/--approx-mapping to generate mappings,\n"
                    "[wfmash] then align them with: wfmash ... -i mappings.paf\n");
    return 1;
  }
  if ((uint64_t)mp.window_length >= mp.max_mapping_length) {  // parse_args.hpp:485-488
    fprintf(stderr, "[wfmash] ERROR, skch::parseandSave, window size should not be larger than max mapping length.\n");
    return 1;
  }
  if ((uint64_t)mp.block_length >= mp.max_mapping_length) {  // :489-492
    fprintf(stderr, "[wfmash] ERROR, skch::parseandSave, block length should not be larger than max mapping length.\n");
    return 1;
  }
  // what the align phase derives from the segment length (parse_args.hpp:590-591, :600-620): the paddings default to
  // it, capped at 5000, and a mapping may be at most 128 segments long on its shorter axis
  if (!target_padding_given) ap.target_padding = (uint64_t)std::min<int64_t>(mp.window_length, 5000);
  if (!query_padding_given) ap.query_padding = (uint64_t)std::min<int64_t>(mp.window_length, 5000);
  ap.wflign_max_len_minor = (uint64_t)mp.window_length * 128;
  const bool hand_off = mapping_in.empty() && !approx_only;  // a temporary mapping file between the phases
  const std::string tmp_dir = tmp_base.empty() ? "." : tmp_base;
  if (hand_off && !tmp_base.empty()) {  // checked before any device is opened
    struct stat sb;
    if (stat(tmp_dir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode) || access(tmp_dir.c_str(), W_OK | X_OK) != 0) {
      fprintf(stderr, "[wfmash] ERROR: the temporary directory (-B) %s does not exist or is not writable\n", tmp_dir.c_str());
      return 1;
    }
  }
  const char* q = query.empty() ? nullptr : query.c_str();
  auto seed = [&](const std::string& to) {  // -K: the seeds through the filters into `to` (host only)
    wfmh_map_summary_t ms;
    const int rc = wfmh_seed_paf(target.c_str(), q, seeds_in.c_str(), to.c_str(), &mp, &ms);
    if (rc == WFM_OK)
      fprintf(stderr, "[wfmash::seeds] %llu seeds of %llu queries -> %llu records; reading %.0f ms, filtering %.0f ms, total %.0f ms\n",
              (unsigned long long)ms.l2_mappings, (unsigned long long)ms.queries, (unsigned long long)ms.written, ms.ms_map, ms.ms_filter, ms.ms_total);
    return rc;
  };
  if (!seeds_in.empty() && approx_only) return seed(out) == WFM_OK ? 0 : 3;
  // one handle per GPU; every phase hands its batches to whichever device is free
  if (gpus == 0) { gpus = wfm_device_count() - device; if (gpus < 1) gpus = 1; }
  std::vector<wfm_handle_t*> hs;
  for (int g = 0; g < gpus; ++g) {
    wfm_handle_t* hg = nullptr;
    if (wfm_create(device + g, &hg) != WFM_OK) {
      fprintf(stderr, "[wfmash] ERROR: no usable MI355X device %d (there is no CPU fallback)\n", device + g);
      for (wfm_handle_t* o : hs) wfm_destroy(o);
      return 2;
    }
    hs.push_back(hg);
  }
  wfm_handle_t* h = hs.front();
  auto destroy_all = [&] { for (wfm_handle_t* o : hs) wfm_destroy(o); };
  if (ani_only) {  // the table and nothing else: no index, no mapping, no PAF
    const int arc = wfmh_ani_matrix(hs.data(), (int)hs.size(), target.c_str(), q, &mp, ani_matrix_out.c_str());
    if (arc == WFM_OK) fprintf(stderr, "[wfmash::ani] table written to %s\n", ani_matrix_out.c_str());
    else fprintf(stderr, "[wfmash::ani] ERROR: %s\n", wfm_last_error(h));
    destroy_all();
    return arc == WFM_OK ? 0 : 3;
  }
  if (!ani_matrix_out.empty()) wfmh_set_ani_matrix(ani_matrix_out.c_str());  // the map call below writes it before it maps
  int rc = WFM_OK;
  std::string mapping = mapping_in;
  std::string temp;
  if (mapping.empty()) {
    if (approx_only) mapping = out;
    else {  // the hand-off file between the phases (temp_file::create, parse_args.hpp:805-808; temp_file.hpp:66-105)
      std::string tmpl = tmp_dir + "/wfmash-XXXXXX";
      const int fd = mkstemp(&tmpl[0]);
      if (fd < 0) { fprintf(stderr, "[wfmash] ERROR: cannot create a temporary file in %s\n", tmp_dir.c_str()); destroy_all(); return 1; }
      close(fd);
      temp = tmpl;
      mapping = temp;
    }
  }
  if (!seeds_in.empty()) {
    rc = seed(mapping);  // then aligned exactly as the mapper's hand-off file is
  } else if (mapping_in.empty()) {
    wfmh_map_summary_t ms;
    rc = wfmh_map_multi(hs.data(), (int)hs.size(), target.c_str(), q, mapping.c_str(), &mp, &ms);
    if (rc == WFM_OK)
      fprintf(stderr, "[wfmash::map] %llu queries x %llu targets (%llu subsets), identity %.2f%%, sketch %d: %llu fragments, %llu segment mappings, "
                      "%llu records; index %.0f ms (+ %.0f ms to copy it to the other GPUs), mapping %.0f ms, filtering %.0f ms, total %.0f ms\n",
              (unsigned long long)ms.queries, (unsigned long long)ms.targets, (unsigned long long)ms.subsets, ms.percentage_identity * 100.0,
              ms.sketch_size, (unsigned long long)ms.fragments, (unsigned long long)ms.l2_mappings, (unsigned long long)ms.written, ms.ms_index, ms.ms_replicate,
              ms.ms_map, ms.ms_filter, ms.ms_total);
    else fprintf(stderr, "[wfmash::map] ERROR: %s\n", wfm_last_error(h));
  }
  auto release_temp = [&] {  // -Z: kept (temp_file.hpp:42)
    if (temp.empty()) return;
    if (keep_temp) fprintf(stderr, "[wfmash] keeping temporary file %s\n", temp.c_str());
    else unlink(temp.c_str());
  };
  if (mp.index_file && mp.write_index) {  // -W: "index construction completed", nothing else runs (computeMap.hpp:405-415)
    release_temp();
    destroy_all();
    return rc == WFM_OK ? 0 : 3;
  }
  bool verify_failed = false;
  if (rc == WFM_OK && !approx_only) {
    wfmh_align_summary_t s;
    if (verify) wfmh_set_verify(1);
    if (verify_optimal) wfmh_set_verify_optimal(1, verify_optimal_cells);
    if (left_align) wfmh_set_left_align(1);
    if (cs_form) wfmh_set_cs(cs_form);
    if (!variants_out.empty()) wfmh_set_variants(variants_out.c_str());
    if (!genotypes_out.empty()) wfmh_set_genotypes(genotypes_out.c_str());
    if (!coverage_out.empty()) wfmh_set_coverage(coverage_out.c_str());
    if (!lift_bed.empty()) wfmh_set_lift(lift_bed.c_str(), lift_out.c_str());
    if (!chain_out.empty()) wfmh_set_chain(chain_out.c_str(), chain_swap ? 1 : 0);
    if (!chain_net_out.empty()) wfmh_set_chain_net(chain_net_out.c_str());
    if (!maf_out.empty()) wfmh_set_maf(maf_out.c_str(), (uint32_t)std::max<int64_t>(0, maf_split));
    if (!trans_bed.empty()) wfmh_set_transitive(trans_bed.c_str(), trans_out.c_str(), (uint32_t)trans_depth);
    if (pav_on) wfmh_set_pav(pav_bed.empty() ? nullptr : pav_bed.c_str(), pav_window, pav_out.c_str());
    rc = wfmh_align_paf_multi(hs.data(), (int)hs.size(), target.c_str(), q, mapping.c_str(), out.c_str(), &ap, &s);
    if (rc == WFM_OK)
      fprintf(stderr, "[wfmash::align] %llu records, %llu aligned bp, %.1f ms GPU kernels, %.1f ms total => %.3g aligned bp/s\n",
              (unsigned long long)s.records, (unsigned long long)s.aligned_bp, s.ms_gpu, s.ms_total, s.aligned_bp / (s.ms_total * 1e-3));
    else fprintf(stderr, "[wfmash::align] ERROR: %s\n", wfm_last_error(h));
    if (left_align && rc == WFM_OK) {
      uint64_t lc[4] = {0, 0, 0, 0};
      wfmh_left_align_counts(lc);
      fprintf(stderr, "[wfmash::left-align] %llu records, %llu interior gaps, %llu moved, %llu records left alone\n", (unsigned long long)lc[0],
              (unsigned long long)lc[1], (unsigned long long)lc[2], (unsigned long long)lc[3]);
    }
    if (cs_form && rc == WFM_OK) {
      uint64_t cc[4] = {0, 0, 0, 0};
      wfmh_cs_counts(cc);
      fprintf(stderr, "[wfmash::cs] %llu records, %llu bytes (%s), %llu records left without a string\n", (unsigned long long)cc[0], (unsigned long long)cc[1],
              cs_form == 2 ? "long" : "short", (unsigned long long)cc[2]);
    }
    if (!variants_out.empty() && rc == WFM_OK) {
      uint64_t vc[4] = {0, 0, 0, 0};
      wfmh_variants_counts(vc);
      fprintf(stderr, "[wfmash::variants] %llu records, %llu variants written, %llu SNVs masked, %llu records left alone\n", (unsigned long long)vc[0],
              (unsigned long long)vc[1], (unsigned long long)vc[2], (unsigned long long)vc[3]);
    }
    if (!genotypes_out.empty() && rc == WFM_OK) {
      uint64_t gc[4] = {0, 0, 0, 0};
      wfmh_genotypes_counts(gc);
      fprintf(stderr, "[wfmash::genotypes] %llu records added, %llu sites written, %llu variants merged away, %llu records left alone\n", (unsigned long long)gc[0],
              (unsigned long long)gc[1], (unsigned long long)gc[2], (unsigned long long)gc[3]);
    }
    if (pav_on && rc == WFM_OK) {
      uint64_t pc[4] = {0, 0, 0, 0};
      wfmh_pav_counts(pc);
      fprintf(stderr, "[wfmash::pav] %llu records added, %llu rows written, %llu union intervals, %llu BED lines skipped\n", (unsigned long long)pc[0],
              (unsigned long long)pc[1], (unsigned long long)pc[2], (unsigned long long)pc[3]);
    }
    if (!lift_bed.empty() && rc == WFM_OK) {
      uint64_t lc[4] = {0, 0, 0, 0};
      wfmh_lift_counts(lc);
      fprintf(stderr, "[wfmash::lift] %llu records lifted, %llu lines written, %llu of them empty, %llu BED lines skipped\n", (unsigned long long)lc[0],
              (unsigned long long)lc[1], (unsigned long long)lc[2], (unsigned long long)lc[3]);
    }
    if (!chain_out.empty() && rc == WFM_OK) {
      uint64_t hc[4] = {0, 0, 0, 0};
      wfmh_chain_counts(hc);
      fprintf(stderr, "[wfmash::chain] %llu chains written, %llu blocks, %llu records refused\n", (unsigned long long)hc[0], (unsigned long long)hc[1],
              (unsigned long long)hc[2]);
    }
    if (!chain_net_out.empty() && rc == WFM_OK) {
      uint64_t nc[4] = {0, 0, 0, 0};
      wfmh_chain_net_counts(nc);
      fprintf(stderr, "[wfmash::chain-net] %llu records added, %llu chains written, %llu pieces, %llu records won nothing\n", (unsigned long long)nc[0],
              (unsigned long long)nc[1], (unsigned long long)nc[2], (unsigned long long)nc[3]);
    }
    if (!maf_out.empty() && rc == WFM_OK) {
      uint64_t mc[4] = {0, 0, 0, 0};
      wfmh_maf_counts(mc);
      fprintf(stderr, "[wfmash::maf] %llu records, %llu blocks, %llu columns, %llu records left without blocks\n", (unsigned long long)mc[0], (unsigned long long)mc[1],
              (unsigned long long)mc[2], (unsigned long long)mc[3]);
    }
    if (!trans_bed.empty() && rc == WFM_OK) {
      uint64_t tc[4] = {0, 0, 0, 0};
      wfmh_transitive_counts(tc);
      fprintf(stderr, "[wfmash::transitive] %llu records added, %llu lines written, %llu rounds, %llu BED lines skipped\n", (unsigned long long)tc[0],
              (unsigned long long)tc[1], (unsigned long long)tc[2], (unsigned long long)tc[3]);
    }
    if (!coverage_out.empty() && rc == WFM_OK) {
      uint64_t cc[4] = {0, 0, 0, 0};
      wfmh_coverage_counts(cc);
      fprintf(stderr, "[wfmash::coverage] %llu records added, %llu bases covered, sum of depth %llu, %llu intervals written\n", (unsigned long long)cc[0],
              (unsigned long long)cc[1], (unsigned long long)cc[2], (unsigned long long)cc[3]);
    }
    if (verify && rc == WFM_OK) {  // everything has been written by now
      uint64_t vc[4] = {0, 0, 0, 0};
      wfmh_verify_counts(vc);
      fprintf(stderr, "[wfmash::verify] %llu lines checked, %llu failed, %llu unverifiable, %llu bases compared\n", (unsigned long long)vc[0],
              (unsigned long long)vc[1], (unsigned long long)vc[2], (unsigned long long)vc[3]);
      verify_failed = vc[1] != 0;
    }
    if (verify_optimal && rc == WFM_OK) {
      uint64_t oc[4] = {0, 0, 0, 0};
      wfmh_verify_optimal_counts(oc);
      fprintf(stderr, "[wfmash::verify] optimal: %llu problems checked, %llu failed, %llu skipped (over the cell cap), %llu cells\n", (unsigned long long)oc[0],
              (unsigned long long)oc[1], (unsigned long long)oc[2], (unsigned long long)oc[3]);
      verify_failed = verify_failed || oc[1] != 0;
    }
  }
  release_temp();
  destroy_all();
  return rc == WFM_OK && !verify_failed ? 0 : 3;
}
