// depth_internal.h - what depth_host.cpp (the two entry points, the files) and depth.hip (the kernels) share.  The rules are those
// of include/hylight_mi.h (hlmi_depth, hlmi_depth_reads); tests/depth_model.py restates them.
#pragma once
#include <vector>

#include "common.h"
#include "depth_text.h"
#include "polish_internal.h"

namespace hlmi {
namespace depth {

// Everything is device memory except h_cbase.  spans: the selected rows as (contig record, ts, te) in the order (contig, ts,
// line); tiles, cbase: polish_layout's (the tile is pol::POLISH_TILE), over the contigs with a selected row ("slots").
struct DepthCoreIn {
    const pol::PolSpan *spans = nullptr;
    size_t n_spans = 0;
    const pol::PolTile *tiles = nullptr;
    size_t n_tiles = 0;
    const uint32_t *cbase = nullptr;
    const std::vector<uint32_t> *h_cbase = nullptr;     // the same on the host: n_slots + 1 entries, the last one the total
    bool want_runs = false;
};
// depth per position (stays in HBM), covered and the sum per slot, the median per slot, and the runs when asked for
void depth_core(const DepthCoreIn &in, DeviceDepth &out);

// hlmi_depth_reads: a thread per selected row writes its span straight from the overlapper's record
void depth_spans_from_rows(const PafRec *recs, const uint32_t *idx, size_t n_sel, const uint32_t *crec_of_rank, pol::PolSpan *out);

}  // namespace depth

// pairs_paf, out_bedgraph: may be nullptr
void depth_run(const char *contigs, const char *reads, const char *paf, const hlmi_depth_opts &o, const char *pairs_paf,
               const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st);
void depth_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_depth_opts &o, const char *pairs_paf,
                     const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st);

}  // namespace hlmi
