// phase_internal.h - what phase_host.cpp, phase_ins_host.cpp (the entry points, the files), phase.hip, phase_reach.hip and
// phase_ins.hip (the kernels) share.  The
// rules are those of include/hylight_mi.h (hlmi_phase, hlmi_phase_reads, hlmi_phase_reach, hlmi_phase_reads_reach, hlmi_phase_ins,
// hlmi_phase_reads_ins); tests/phase_model.py, tests/phase_reach_model.py and tests/phase_ins_model.py restate them.
#pragma once
#include <vector>

#include "common.h"
#include "phase_ins_text.h"
#include "phase_reach_text.h"
#include "phase_text.h"
#include "polish_internal.h"
#include "polish_select.h"
#include "variants_internal.h"

namespace hlmi {
namespace ph {

constexpr int PHASE_TILE = 1024;        // links per workgroup of the link pass (tests read this line)
constexpr int PHASE_REACH_TILE = 512;   // left sites per workgroup of the link pass over every distance (tests read this line)

struct DevicePhase {
    std::vector<LinkCounts> links;      // one per pair of neighbouring sites, those across a contig junction included (zeros)
    Blocks blocks;
    std::vector<ReadRec> recs;          // rows ascending, a row's blocks ascending
    uint64_t alleles = 0;               // bytes of the allele table
    // reach >= 1 (hlmi_phase_reach): the links of every distance (far.reach: 0 in a plain call) and what build_blocks_reach counted
    ReachLinks far;
    uint64_t links_far = 0, links_far_phased = 0, joins_far = 0, sites_bridged = 0, links_conflict = 0;
};

// the rows [row_lo, row_hi) that can hold a link of a tile of links
struct LinkTile {
    uint32_t row_lo, row_hi;
};
// The rows of every tile of `tile` links (a link belongs to its left site) from the rows' site ranges: from the first row that
// holds a link of the tile or a later one to the last row that starts in front of the tile's end (s_lo ascends with the rows).
std::vector<LinkTile> link_tiles(const std::vector<uint32_t> &s_lo, const std::vector<uint32_t> &cnt, size_t n_links, size_t tile);
// refuses what does not fit the device's free memory, under the entry point's name
void check_fits(const char *who, const char *what, uint64_t bytes);
// phase_reach.hip: the counters of the links (j, j + d), 1 <= d <= out.reach, of the n_links left sites, over the allele table
// (s_lo, cnt, off, table in device memory; h_lo and h_cnt the first two on the host).  16 * reach bytes per left site come down.
void link_reach(const char *who, const std::vector<uint32_t> &h_lo, const std::vector<uint32_t> &h_cnt, size_t n_links, const uint32_t *s_lo,
                const uint32_t *cnt, const uint64_t *off, const uint8_t *table, ReachLinks &out);

// The device part behind variants_core, over the same input: the allele table of the rows at `sites` (ascending by gpos), the
// link counters, the blocks (built on the host between two kernels: phase_text.h) and the records per (row, block).  No site: no
// kernel is launched.  who: the entry point's name in the refusal of a table of 2^32 bytes or of more than the device holds.
// keep (hlmi_haplotigs): the records stay in device memory as well, with every row's first record and number of records.
// reach: 0 for the plain calls (links between neighbours, phase_link_kernel, build_blocks); 1 .. PHASE_REACH_MAX for the _reach
// calls (phase_link_reach_kernel, build_blocks_reach, bridged sites left out of a record's hap_a, hap_b and other).
struct DevRecs {
    DBuf<ReadRec> recs;
    DBuf<uint64_t> off;                 // per row
    DBuf<uint32_t> cnt;
    uint64_t n = 0;
};
void phase_core(const char *who, const pol::PolCoreIn &in, const std::vector<PSite> &sites, const hlmi_phase_opts &o, DevicePhase &out,
                DevRecs *keep = nullptr, int reach = 0);

// phase_core behind its allele table, shared with phase_ins_core: the link pass over the table (s_lo, cnt, off, table of the R
// rows in device memory; no site or no allele: not read), the blocks, the records.  out.alleles and out.far.reach are the caller's
void phase_tail(const char *who, size_t R, const std::vector<PSite> &sites, const hlmi_phase_opts &o, DevicePhase &out, DevRecs *keep, int reach,
                const DBuf<uint32_t> &s_lo, const DBuf<uint32_t> &cnt, const DBuf<uint64_t> &off, const DBuf<uint8_t> &table);
// phase_ins.hip (hlmi_phase_ins): phase_core over the merged list of position and insertion sites, 1 <= reach <= PHASE_REACH_MAX:
// the table's front by kind (an I op's length against the site's at a slot), then phase_tail.  keep (hlmi_haplotigs_ins): as
// phase_core's
void phase_ins_core(const char *who, const pol::PolCoreIn &in, const MergedSites &M, const hlmi_phase_opts &o, DevicePhase &out, int reach,
                    DevRecs *keep = nullptr);

// the query name rank of every selected row of the overlapper's rows (recs[idx[j]].qid): 4 bytes per row come down
std::vector<uint32_t> selected_query_ranks(const PafRec *recs, const uint32_t *idx, size_t n_sel);

// ---- what the entry points do around phase_core (phase_host.cpp); hlmi_haplotigs calls the same functions -----------------------
// the option refusals, in the header's order: hlmi_variants's (check_variant_opts), min_link, min_agree
void check_phase_opts(const char *who, const hlmi_phase_opts &o);
// ... and behind them a _reach call's: reach < 1 or > HLMI_PHASE_REACH_MAX
void check_reach(const char *who, int reach);
struct Phased {
    var::DeviceVariants var;
    std::vector<PSite> sites;
    DevicePhase dev;
};
// the device part over the rows of the front (R.up.core): hlmi_variants's sites, then the phasing
void phase_device(const char *who, const pol::PileupRows &R, const hlmi_phase_opts &o, Phased &P, DevRecs *keep = nullptr, int reach = 0);
// what follows the device part: the statistics and the three files.  rows_read: R.read_of_row(), needed (and asked for) only when
// out_reads has a line to write.  out_sites == nullptr (hlmi_haplotigs): the statistics alone.  Behind a phase_device with
// reach >= 1 the sites file has "." at a bridged site and the links file the links of every distance; far (may be nullptr)
// takes the five counters of hlmi_phase_reach_stats
void phase_emit(const char *who, const pol::PileupRows &R, const Phased &P, const hlmi_phase_opts &o, const std::vector<uint32_t> &rows_read,
                const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st,
                hlmi_phase_reach_stats *far = nullptr);

}  // namespace ph

// pairs_paf, out_links, out_reads: may be nullptr
void phase_run(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts &o, const char *pairs_paf,
               const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);
void phase_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_phase_opts &o, const char *pairs_paf,
                     const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);
void phase_reach_run(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts &o, int reach, const char *pairs_paf,
                     const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_reach_stats *st);
void phase_reads_reach_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_phase_opts &o, int reach,
                           const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads,
                           hlmi_phase_reach_stats *st);
// phase_ins_host.cpp
void phase_ins_run(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts &o, int reach, const char *pairs_paf,
                   const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_ins_stats *st);
void phase_reads_ins_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_phase_opts &o, int reach,
                         const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads,
                         hlmi_phase_ins_stats *st);

}  // namespace hlmi
