// The text side of --genotypes (wfmash_amd/host/genotype_text.hpp) on its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/micro/genotypes_check.cpp -o /tmp/genotypes_check && /tmp/genotypes_check
// header with and without groups and sequences; line on rows of every cell kind, without groups, with alleles at the very end of their
// buffer; order on ties at one pos in every permutation, on a list that does not ascend, on one site and on none; sequence_of at the
// first and last base of every sequence, with empty sequences between them; site_line at the last base of the last sequence.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../wfmash_amd/host/genotype_text.hpp"

static int fails = 0;
static void expect_text(const std::string& got, const std::string& want, const char* what) {
  if (got != want) { fprintf(stderr, "FAIL %s: got\n%swant\n%s", what, got.c_str(), want.c_str()); ++fails; }
}
static void expect(bool ok, const char* what) {
  if (!ok) { fprintf(stderr, "FAIL %s\n", what); ++fails; }
}

int main() {
  const std::string head =
      "##fileformat=VCFv4.2\n##source=wfmash-hip 9.9\n##contig=<ID=t#1#a,length=100>\n##contig=<ID=t#1#b,length=50>\n"
      "##INFO=<ID=QNAME,Number=1,Type=String,Description=\"Query sequence name\">\n"
      "##INFO=<ID=QSTART,Number=1,Type=Integer,Description=\"Start of the query bases in ALT, 0-based, forward strand\">\n"
      "##INFO=<ID=QEND,Number=1,Type=Integer,Description=\"End of the query bases in ALT, exclusive, forward strand\">\n"
      "##INFO=<ID=QSTRAND,Number=1,Type=String,Description=\"Strand of the query in the alignment\">\n"
      "##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Groups that carry ALT\">\n"
      "##INFO=<ID=AN,Number=1,Type=Integer,Description=\"Groups with a called allele, REF or ALT\">\n"
      "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Haploid genotype of the group: 1 carries ALT, 0 has REF under = bases, . neither\">\n"
      "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
  expect_text(genotype::header("9.9", {"t#1#a", "t#1#b"}, {100, 50}, {"q#1", "q#2"}), head + "\tq#1\tq#2\n", "header");
  expect_text(genotype::header("9.9", {"t#1#a", "t#1#b"}, {100, 50}, {}), head + "\n", "header without groups");
  expect(genotype::header("x", {}, {}, {}).find("##contig") == std::string::npos, "header without sequences");

  // the alleles lie at the very end of a heap block of exactly their size: a read past them is the sanitizer's
  {
    std::vector<char> a = {'A', 'A', 'C', 'G'};  // REF A, ALT ACG
    std::vector<char> cells = {'1', '0', '.', '1'};
    std::string out;
    genotype::line(out, "chr", 7, a.data(), 1, a.data() + 1, 3, cells.data(), cells.size());
    expect_text(out, "chr\t7\t.\tA\tACG\t.\t.\tAC=2;AN=3\tGT\t1\t0\t.\t1\n", "line");
    out.clear();
    genotype::line(out, "chr", 18446744073709551615ull, a.data(), 1, a.data() + 1, 3, cells.data(), 0);
    expect_text(out, "chr\t18446744073709551615\t.\tA\tACG\t.\t.\tAC=0;AN=0\tGT\n", "line without groups, the largest POS");
  }

  // ties at one pos: REF bytes, then ALT bytes, bytewise (a prefix first, high bytes last), in every order they may come in
  {
    struct A { const char* ref; const char* alt; };
    const std::vector<A> want = {{"A", "AG"}, {"A", "AGG"}, {"A", "G"}, {"A", "T"}, {"A", "\xc3"}, {"AC", "A"}, {"ACG", "A"}};
    std::vector<size_t> perm(want.size());
    for (size_t i = 0; i < perm.size(); ++i) perm[i] = i;
    int rounds = 0;
    do {
      std::vector<char> alleles;
      std::vector<genotype::Site> sites;
      sites.push_back(genotype::Site{3, 1, 1, 0});
      alleles.push_back('C'); alleles.push_back('T');
      for (size_t k : perm) {
        const std::string r = want[k].ref, a = want[k].alt;
        sites.push_back(genotype::Site{10, (uint32_t)r.size(), (uint32_t)a.size(), (uint64_t)alleles.size()});
        alleles.insert(alleles.end(), r.begin(), r.end());
        alleles.insert(alleles.end(), a.begin(), a.end());
      }
      sites.push_back(genotype::Site{11, 1, 1, 0});
      const std::vector<size_t> idx = genotype::order(sites, alleles.data());
      bool ok = idx.size() == sites.size() && idx.front() == 0 && idx.back() == sites.size() - 1;
      for (size_t j = 0; ok && j < want.size(); ++j) ok = perm[idx[1 + j] - 1] == j;
      if (!ok) { expect(false, "order of the ties"); break; }
      ++rounds;
    } while (std::next_permutation(perm.begin(), perm.end()) && rounds < 5040);
    expect(rounds == 5040, "all the permutations of seven ties");
  }
  {
    const std::vector<char> alleles = {'A', 'C'};
    const std::vector<genotype::Site> down = {{9, 1, 1, 0}, {5, 1, 1, 0}, {7, 1, 1, 0}};
    expect(genotype::order(down, alleles.data()) == std::vector<size_t>({1, 2, 0}), "a list that does not ascend");
    expect(genotype::order({{9, 1, 1, 0}}, alleles.data()) == std::vector<size_t>({0}), "one site");
    expect(genotype::order({}, nullptr).empty(), "no site");
  }

  // sequences of 100, 0, 0, 50 and 1 bases
  {
    const std::vector<uint64_t> off = {0, 100, 100, 100, 150, 151};
    expect(genotype::sequence_of(off, 0) == 0 && genotype::sequence_of(off, 99) == 0, "sequence_of: the first sequence");
    expect(genotype::sequence_of(off, 100) == 3 && genotype::sequence_of(off, 149) == 3, "sequence_of: behind two empty sequences");
    expect(genotype::sequence_of(off, 150) == 4, "sequence_of: the last base");
    const std::vector<std::string> names = {"a", "e1", "e2", "b", "c"};
    std::vector<char> alleles = {'G', 'T'}, gt = {'.', '1'};
    const std::vector<genotype::Site> sites = {{150, 1, 1, 0}};
    std::string out;
    genotype::site_line(out, sites, 0, alleles.data(), gt.data(), 2, names, off);
    expect_text(out, "c\t1\t.\tG\tT\t.\t.\tAC=1;AN=1\tGT\t.\t1\n", "site_line at the last base");
  }
  if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
  printf("genotypes_check: ok\n");
  return 0;
}
