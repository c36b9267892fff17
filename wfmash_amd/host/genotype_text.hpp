// genotype_text.hpp -- the text side of --genotypes: the VCF header with one column per group, the order of the lines and the lines.  Pure
// host code on the standard library alone, so that it can be built on its own (scripts/micro/genotypes_check.cpp runs it under the
// address and undefined-behaviour sanitizers).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace genotype {

// a site as wfm_sites_table returns it: pos over the concatenation of the target's sequences, REF = alleles[off .. off + ref_len), ALT
// the alt_len bytes behind
struct Site {
  uint64_t pos;
  uint32_t ref_len, alt_len;
  uint64_t off;
};

// --variants' header lines, AC and AN, GT, and the column line with one column per group
inline std::string header(const std::string& version, const std::vector<std::string>& names, const std::vector<uint64_t>& lengths,
                          const std::vector<std::string>& keys) {
  std::string out = "##fileformat=VCFv4.2\n##source=wfmash-hip " + version + "\n";
  for (size_t i = 0; i < names.size(); ++i) out += "##contig=<ID=" + names[i] + ",length=" + std::to_string(lengths[i]) + ">\n";
  out += "##INFO=<ID=QNAME,Number=1,Type=String,Description=\"Query sequence name\">\n"
         "##INFO=<ID=QSTART,Number=1,Type=Integer,Description=\"Start of the query bases in ALT, 0-based, forward strand\">\n"
         "##INFO=<ID=QEND,Number=1,Type=Integer,Description=\"End of the query bases in ALT, exclusive, forward strand\">\n"
         "##INFO=<ID=QSTRAND,Number=1,Type=String,Description=\"Strand of the query in the alignment\">\n"
         "##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Groups that carry ALT\">\n"
         "##INFO=<ID=AN,Number=1,Type=Integer,Description=\"Groups with a called allele, REF or ALT\">\n"
         "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Haploid genotype of the group: 1 carries ALT, 0 has REF under = bases, . neither\">\n"
         "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
  for (const std::string& k : keys) { out += '\t'; out += k; }
  out += '\n';
  return out;
}

inline int compare_bytes(const char* a, size_t na, const char* b, size_t nb) {
  const int c = memcmp(a, b, std::min(na, nb));
  return c ? c : (na < nb ? -1 : na > nb ? 1 : 0);
}

// The order of the lines: (pos, REF bytes, ALT bytes).  The sites come in ascending pos; the few ties at one pos are put in bytewise
// order here, so that the file does not depend on how the device orders them.  Returns the indexes of the sites in file order.
inline std::vector<size_t> order(const std::vector<Site>& sites, const char* alleles) {
  std::vector<size_t> idx(sites.size());
  for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
  auto less = [&](size_t x, size_t y) {
    const Site &a = sites[x], &b = sites[y];
    if (a.pos != b.pos) return a.pos < b.pos;
    if (const int c = compare_bytes(alleles + a.off, a.ref_len, alleles + b.off, b.ref_len)) return c < 0;
    return compare_bytes(alleles + a.off + a.ref_len, a.alt_len, alleles + b.off + b.ref_len, b.alt_len) < 0;
  };
  for (size_t a = 0; a < idx.size();) {
    size_t b = a + 1;
    while (b < idx.size() && sites[idx[b]].pos == sites[idx[a]].pos) ++b;
    if (b - a > 1) std::sort(idx.begin() + (long)a, idx.begin() + (long)b, less);
    a = b;
  }
  if (!std::is_sorted(idx.begin(), idx.end(), less)) std::sort(idx.begin(), idx.end(), less);  // (a list that did not ascend)
  return idx;
}

// the target sequence a global position lies in: the last one that begins at or before it and is not empty.  offsets: nseq + 1 values
inline size_t sequence_of(const std::vector<uint64_t>& offsets, uint64_t pos) {
  size_t c = (size_t)(std::upper_bound(offsets.begin(), offsets.end(), pos) - offsets.begin());
  return c ? c - 1 : 0;
}

// one line: CHROM POS . REF ALT . . AC=a;AN=n GT and the n_groups cells ('0', '1', '.'); a = the 1s of the row, n = its 0s and 1s
inline void line(std::string& out, const std::string& tname, uint64_t pos1, const char* ref, size_t ref_len, const char* alt, size_t alt_len, const char* cells,
                 size_t n_groups) {
  char num[100];
  size_t ac = 0, an = 0;
  for (size_t g = 0; g < n_groups; ++g) { ac += cells[g] == '1'; an += cells[g] == '1' || cells[g] == '0'; }
  out += tname;
  out.append(num, (size_t)snprintf(num, sizeof num, "\t%llu\t.\t", (unsigned long long)pos1));
  out.append(ref, ref_len);
  out += '\t';
  out.append(alt, alt_len);
  out.append(num, (size_t)snprintf(num, sizeof num, "\t.\t.\tAC=%zu;AN=%zu\tGT", ac, an));
  for (size_t g = 0; g < n_groups; ++g) { out += '\t'; out += cells[g]; }
  out += '\n';
}

// the line of site i of the table (gt: n_sites x n_groups cells, row-major)
inline void site_line(std::string& out, const std::vector<Site>& sites, size_t i, const char* alleles, const char* gt, size_t n_groups,
                      const std::vector<std::string>& names, const std::vector<uint64_t>& offsets) {
  const Site& s = sites[i];
  const size_t c = sequence_of(offsets, s.pos);
  line(out, names[c], s.pos - offsets[c] + 1, alleles + s.off, s.ref_len, alleles + s.off + s.ref_len, s.alt_len, gt + i * n_groups, n_groups);
}

// The file of --genotypes from the table of a sites object (Raw: wfm_site_t, or anything with Site's fields): the header, then the sites'
// lines in order()'s order; gt: n_sites x keys.size() cells.  The text goes to `out` (anything that takes << of a string) a MiB at a time.
template <class Sink, class Raw>
inline void vcf(Sink& out, const std::string& version, const std::vector<std::string>& names, const std::vector<uint64_t>& lengths,
                const std::vector<uint64_t>& offsets, const std::vector<std::string>& keys, const Raw* rows, size_t n_sites, const char* alleles, const char* gt) {
  std::vector<Site> sites(n_sites);
  for (size_t i = 0; i < n_sites; ++i) sites[i] = Site{rows[i].pos, rows[i].ref_len, rows[i].alt_len, rows[i].off};
  std::string text = header(version, names, lengths, keys);
  for (size_t i : order(sites, alleles)) {
    site_line(text, sites, i, alleles, gt, keys.size(), names, offsets);
    if (text.size() >= ((size_t)1 << 20)) { out << text; text.clear(); }
  }
  out << text;
}

}  // namespace genotype
