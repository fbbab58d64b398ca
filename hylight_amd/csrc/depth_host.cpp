// depth_host.cpp - the host part of hlmi_depth and hlmi_depth_reads (include/hylight_mi.h): read depth and relative abundance per
// contig.  The rows come from the pile-up calls' row front (polish_select.h), asked for spans only: the selected rows' spans, the
// covered contigs' tiles and cbase, nothing else.  The depths, medians and runs are depth.hip's, the records and the text
// depth_text.h's.
// PARITY UNPINNED: a function of the project's own; tests/depth_model.py is the contract.
#include <string>
#include <vector>

#include "ava.h"
#include "common.h"
#include "depth_internal.h"
#include "paf_io.h"
#include "polish_internal.h"
#include "polish_select.h"

namespace hlmi {

using namespace pol;
using namespace depth;

namespace {

// what both entry points do behind the rows: the depths, medians and runs, the records, the statistics and the two files
void depth_body(const PileupRows &R, const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st) {
    const SeqSet &cs = R.cs();
    const PolLayout &L = R.L;
    set_row_stats(R, st);
    DeviceDepth dev;
    if (R.n_sel) {
        DepthCoreIn in;
        in.spans = R.d_spans.p; in.n_spans = R.n_sel;
        in.tiles = R.up.core.tiles; in.n_tiles = L.tiles.size();
        in.cbase = R.up.core.cbase; in.h_cbase = &L.cbase;
        in.want_runs = out_bedgraph != nullptr;
        depth_core(in, dev);
    }
    st->ms_device = now_ms() - R.t_dev;

    std::vector<uint64_t> length(cs.size());
    for (size_t c = 0; c < cs.size(); ++c) length[c] = cs.len(c);
    DepthTotals tot;
    const std::vector<ContigDepth> recs = contig_records(cs.names, length, L.rc, L.slot_of_contig, dev, &tot);
    st->contigs_covered = tot.contigs_covered;
    st->positions = tot.positions;
    st->covered = tot.covered;
    st->bases = tot.bases;
    const std::vector<std::string> tsv = tsv_lines(recs);
    std::vector<std::string> bed;
    if (out_bedgraph) {
        bed = bedgraph_lines(cs.names, length, L.rc, L.slot_of_contig, L.cbase, dev);
        st->runs = bed.size();
    }
    write_lines(out_tsv, tsv);
    if (out_bedgraph) write_lines(out_bedgraph, bed);
}

}  // namespace

void depth_run(const char *contigs, const char *reads, const char *paf, const hlmi_depth_opts &o, const char *pairs_paf,
               const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st) {
    timed_call(st, true, [&] {
        PileupRows R;
        rows_from_paf(contigs, reads, paf, plain_request("hlmi_depth", o.min_len, o.min_iden, pairs_paf, true), R);
        depth_body(R, out_tsv, out_bedgraph, st);
    });
}

void depth_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_depth_opts &o, const char *pairs_paf,
                     const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st) {
    timed_call(st, true, [&] {
        PileupRows R;
        rows_from_reads(contigs, reads, ao, plain_request("hlmi_depth_reads", o.min_len, o.min_iden, pairs_paf, true), R);
        depth_body(R, out_tsv, out_bedgraph, st);
    });
}

}  // namespace hlmi
