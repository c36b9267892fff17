// verify_paf.hpp -- every aligned PAF line held against the bases it names (--verify, --verify-paf).
//
// A line is parsed on its own (names, coordinates as written, strand, cg:Z:), turned into a problem by reference -- pattern =
// target [ts, te), text = query [qs, qe), reverse-complemented for '-' -- and its CIGAR into runs (= M, X X, I I, D D); batches
// of lines go through wfm_upload_sequence_refs and wfm_check_runs (include/wfmash_hip.h), which compares every base on the device.
// What the check sees is the finished line: the record after patching, erosion and swizzle.  Optimality is not checked.
#pragma once

#include <cstdint>
#include <functional>
#include <ostream>
#include <string>
#include <vector>

#include "../../include/wfmash_hip.h"
#include "fasta.hpp"
#include "verify_parse.hpp"

namespace verify {

struct Counts { uint64_t checked = 0, failed = 0, unverifiable = 0, bases = 0; };

// where the bases come from: the two files and, with a sequence store, the id of a whole sequence in it (-1: by host pointer)
struct Source {
  const wfmash_host::FastaStore* target = nullptr;
  const wfmash_host::FastaStore* query = nullptr;
  const wfm_seqstore_t* store = nullptr;
  std::function<int32_t(const wfmash_host::FastaStore*, int)> resident_id;
  int threads = 1;  // host threads the windows that go by host pointer are fetched on
};

// Verifies the lines of `text` (separated by '\n'; empty lines are passed over) on h and adds to `c`; a failure is one line on
// stderr.  Throws std::runtime_error when a device call fails.
void verify_text(wfm_handle_t* h, const Source& src, const std::string& text, Counts& c);

// --maf-paf: the MAF blocks (maf_text.hpp; wfm_maf_rows, split as there) of the lines of `text` to `out`, lines parsed and their windows
// uploaded as verify_text does.  counts += {records written with blocks, blocks, columns, records left without blocks}; skipped +=
// {lines without an =XID cg:Z:, malformed, with a target the target file or a query the query file does not have, with another length}.  Throws when a device call fails.
void maf_text(wfm_handle_t* h, const Source& src, const std::string& text, uint32_t split, std::ostream& out, uint64_t counts[4], uint64_t skipped[4]);

// the process-wide switch of --verify and what the runs since it was last set have counted
void set_enabled(bool on);
bool enabled();
void add_counts(const Counts& c);
Counts total_counts();

}  // namespace verify
