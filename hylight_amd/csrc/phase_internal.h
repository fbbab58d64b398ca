// phase_internal.h - what phase_host.cpp (the two entry points, the files) and phase.hip (the kernels) share.  The rules are those
// of include/hylight_mi.h (hlmi_phase, hlmi_phase_reads); tests/phase_model.py restates them.
#pragma once
#include <vector>

#include "common.h"
#include "phase_text.h"
#include "polish_internal.h"
#include "polish_select.h"
#include "variants_internal.h"

namespace hlmi {
namespace ph {

constexpr int PHASE_TILE = 1024;        // links per workgroup of the link pass (tests read this line)

struct DevicePhase {
    std::vector<LinkCounts> links;      // one per pair of neighbouring sites, those across a contig junction included (zeros)
    Blocks blocks;
    std::vector<ReadRec> recs;          // rows ascending, a row's blocks ascending
    uint64_t alleles = 0;               // bytes of the allele table
};

// The device part behind variants_core, over the same input: the allele table of the rows at `sites` (ascending by gpos), the
// link counters, the blocks (built on the host between two kernels: phase_text.h) and the records per (row, block).  No site: no
// kernel is launched.  who: the entry point's name in the refusal of a table of 2^32 bytes or of more than the device holds.
// keep (hlmi_haplotigs): the records stay in device memory as well, with every row's first record and number of records.
struct DevRecs {
    DBuf<ReadRec> recs;
    DBuf<uint64_t> off;                 // per row
    DBuf<uint32_t> cnt;
    uint64_t n = 0;
};
void phase_core(const char *who, const pol::PolCoreIn &in, const std::vector<PSite> &sites, const hlmi_phase_opts &o, DevicePhase &out,
                DevRecs *keep = nullptr);

// the query name rank of every selected row of the overlapper's rows (recs[idx[j]].qid): 4 bytes per row come down
std::vector<uint32_t> selected_query_ranks(const PafRec *recs, const uint32_t *idx, size_t n_sel);

// ---- what the entry points do around phase_core (phase_host.cpp); hlmi_haplotigs calls the same functions -----------------------
// the option refusals, in the header's order: hlmi_variants's (check_variant_opts), min_link, min_agree
void check_phase_opts(const char *who, const hlmi_phase_opts &o);
struct Phased {
    var::DeviceVariants var;
    std::vector<PSite> sites;
    DevicePhase dev;
};
// the device part over the rows of the front (R.up.core): hlmi_variants's sites, then the phasing
void phase_device(const char *who, const pol::PileupRows &R, const hlmi_phase_opts &o, Phased &P, DevRecs *keep = nullptr);
// what follows the device part: the statistics and the three files.  rows_read: R.read_of_row(), needed (and asked for) only when
// out_reads has a line to write.  out_sites == nullptr (hlmi_haplotigs): the statistics alone
void phase_emit(const char *who, const pol::PileupRows &R, const Phased &P, const hlmi_phase_opts &o, const std::vector<uint32_t> &rows_read,
                const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);

}  // namespace ph

// pairs_paf, out_links, out_reads: may be nullptr
void phase_run(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts &o, const char *pairs_paf,
               const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);
void phase_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_phase_opts &o, const char *pairs_paf,
                     const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);

}  // namespace hlmi
