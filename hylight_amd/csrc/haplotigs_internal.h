// haplotigs_internal.h - what haplotigs_host.cpp, haplotigs_ins_host.cpp (the entry points, the files) and haplotigs.hip (the
// kernels) share.  The rules are those of include/hylight_mi.h (hlmi_haplotigs, hlmi_haplotigs_reads, their _reach and _ins
// forms); tests/haplotigs_model.py, tests/haplotigs_reach_model.py and tests/haplotigs_ins_model.py restate them.
#pragma once
#include <string>
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
    std::vector<uint32_t> gfirst, glast;    // the extent in the device's position space; keys: its kf and kl (ph::site_key) there
    std::vector<uint8_t> split;
    bool keys = false;                      // the _ins calls: extents in key space, the key-space instantiations of the kernels
};

// The device part behind phase_core when a block is split: the rows' exclusion intervals from the records phase_core left in
// device memory (recs), the two-sided count pass over polish_layout's tiles, and polish_tail over the two sides side by side - a
// position space of 2 n_contig positions, side B behind side A - with sided slot votes.  cbase: PolLayout::cbase.  out: as
// polish_core's over that space: sym and open_pos count side B's positions from n_contig, start has 2 (cbase.size() - 1) + 1
// entries.  who: the entry point's name in the refusal of an interval table that does not fit the device's free memory.
// blocks.keys: the rows' intervals are 12 bytes (kf, kl, shut side) and position g is inside iff kf <= 2 g + 1 <= kl, slot g iff
// kf <= 2 g <= kl; recs are then phase_ins_core's.
void haplotig_core(const char *who, const pol::PolCoreIn &in, const std::vector<uint32_t> &cbase, const ph::DevRecs &recs,
                   const HapBlocksUp &blocks, pol::PolDevOut &out);

// ---- what the entry points share on the host (haplotigs_host.cpp) -----------------------------------------------------------------
hlmi_phase_opts phase_part(const hlmi_haplotig_opts &o);
// hlmi_phase's option refusals, then min_side < 1
void check_haplotig_opts(const char *who, const hlmi_haplotig_opts &o);
// a block of two or more sites as the records see it: the first and the last position inside its extent, in the device's
// position space; diff: set for a split one
struct HapExtent {
    uint32_t contig;
    bool split;
    uint32_t gfirst, glast;
    uint64_t diff;
};
// The lines of out_fa from the consensus (any: two sides side by side) and the counters of st they carry: records, the split
// counters, the four decision counters, diff_positions.  ext: every block of two or more sites, contigs and blocks ascending
std::vector<std::string> haplotig_records(const char *who, const pol::PileupRows &R, const hlmi_haplotig_opts &o, bool any,
                                          const pol::PolDevOut &out, std::vector<HapExtent> &ext, hlmi_haplotig_stats *st);

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
// haplotigs_ins_host.cpp: ... over the blocks of hlmi_phase_ins's rule, extents in key space
void haplotigs_ins_run(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts &o, int reach, const char *pairs_paf,
                       const char *out_fa, const char *out_blocks, hlmi_haplotig_ins_stats *st);
void haplotigs_reads_ins_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_haplotig_opts &o, int reach,
                             const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_ins_stats *st);

}  // namespace hlmi
