// haplotigs_internal.h - what haplotigs_host.cpp (the two entry points, the files) and haplotigs.hip (the kernels) share.  The rules
// are those of include/hylight_mi.h (hlmi_haplotigs, hlmi_haplotigs_reads); tests/haplotigs_model.py restates them.
#pragma once
#include <vector>

#include "common.h"
#include "haplotigs_text.h"
#include "phase_internal.h"
#include "polish_internal.h"

namespace hlmi {
namespace hap {

constexpr int HAP_TILE = 1024;          // contig positions per workgroup of the two-sided count pass (tests read this line)

// what goes up per block of the call (ReadRec::block indexes all three): 9 bytes
struct HapBlocksUp {
    std::vector<uint32_t> gfirst, glast;    // the extent in the device's position space
    std::vector<uint8_t> split;
};

// The device part behind phase_core when a block is split: the rows' exclusion intervals from the records phase_core left in
// device memory (recs), the two-sided count pass over polish_layout's tiles, and polish_tail over the two sides side by side - a
// position space of 2 n_contig positions, side B behind side A - with sided slot votes.  cbase: PolLayout::cbase.  out: as
// polish_core's over that space: sym and open_pos count side B's positions from n_contig, start has 2 (cbase.size() - 1) + 1
// entries.  who: the entry point's name in the refusal of an interval table that does not fit the device's free memory.
void haplotig_core(const char *who, const pol::PolCoreIn &in, const std::vector<uint32_t> &cbase, const ph::DevRecs &recs,
                   const HapBlocksUp &blocks, pol::PolDevOut &out);

}  // namespace hap

// pairs_paf, out_blocks: may be nullptr
void haplotigs_run(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts &o, const char *pairs_paf,
                   const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);
void haplotigs_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_haplotig_opts &o, const char *pairs_paf,
                         const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);
// ... over the blocks of hlmi_phase_reach's rule
void haplotigs_reach_run(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts &o, int reach, const char *pairs_paf,
                         const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);
void haplotigs_reads_reach_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_haplotig_opts &o, int reach,
                               const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);

}  // namespace hlmi
