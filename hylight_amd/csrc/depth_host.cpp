// depth_host.cpp - the host part of hlmi_depth and hlmi_depth_reads (include/hylight_mi.h): read depth and relative abundance per
// contig.  The selection is the polisher's own (polish_select.h), the layout of the covered contigs and their tiles too
// (polish_layout); the depths, medians and runs are depth.hip's, the records and the text depth_text.h's.
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

// what both entry points do behind the device part: the records, the statistics and the two files
void depth_emit(const SeqSet &cs, const PolLayout &L, const DeviceDepth &dev, const char *out_tsv, const char *out_bedgraph,
                hlmi_depth_stats *st) {
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

void set_pair_stats(const PolPairCall &pc, bool given, hlmi_depth_stats *st) {
    if (!given) return;
    st->pairs_listed = pc.pairs_listed;
    st->pairs_unknown = pc.pairs_unknown;
    st->rows_not_listed = pc.rows_not_listed;
}

}  // namespace

void depth_run(const char *contigs, const char *reads, const char *paf, const hlmi_depth_opts &o, const char *pairs_paf,
               const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st) {
    const double t_begin = now_ms();
    *st = hlmi_depth_stats{};
    stat_reset();
    PolQualCall qc;                             // no floor and no weights: the quality strings are only checked, as hlmi_polish_pairs does
    PolPairCall pc;
    pc.path = pairs_paf;
    PafSelection S;
    select_paf_rows(contigs, reads, paf, o.min_len, o.min_iden, SelectNames{"hlmi_depth", "hlmi_depth", "hlmi_depth", true}, &qc,
                    pairs_paf ? &pc : nullptr, S);
    st->rows = S.pt.recs.size();
    st->contigs = S.cs.size();
    st->rows_selected = S.sel.size();
    set_pair_stats(pc, pairs_paf != nullptr, st);
    std::vector<PolSpan> spans;
    spans.reserve(S.sel.size());
    for (const PafSel &s : S.sel) spans.push_back(PolSpan{s.contig, S.pt.recs[s.line].ts, S.pt.recs[s.line].te});
    PolLayout L;
    polish_layout(S.cs, spans, "hlmi_depth", L, nullptr, false);

    const double t_dev = now_ms();
    DeviceDepth dev;
    if (!spans.empty()) {
        DBuf<PolSpan> d_spans;
        DBuf<PolTile> d_tiles;
        DBuf<uint32_t> d_cbase;
        d_spans.upload(spans);
        d_tiles.upload(L.tiles);
        d_cbase.upload(L.cbase);
        DepthCoreIn in;
        in.spans = d_spans.p; in.n_spans = spans.size();
        in.tiles = d_tiles.p; in.n_tiles = L.tiles.size();
        in.cbase = d_cbase.p; in.h_cbase = &L.cbase;
        in.want_runs = out_bedgraph != nullptr;
        depth_core(in, dev);
    }
    st->ms_device = now_ms() - t_dev;
    depth_emit(S.cs, L, dev, out_tsv, out_bedgraph, st);
    st->ms_total = now_ms() - t_begin;
}

void depth_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_depth_opts &o, const char *pairs_paf,
                     const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st) {
    const double t_begin = now_ms();
    *st = hlmi_depth_stats{};
    stat_reset();
    PolPairCall pc;
    pc.path = pairs_paf;
    RowSelection sel;
    select_device_rows(contigs, reads, ao, o.min_len, o.min_iden,
                       SelectNames{"hlmi_depth_reads", "hlmi_depth_reads", "hlmi_depth_reads", true}, nullptr, pairs_paf ? &pc : nullptr, sel);
    const size_t S = sel.n_sel;
    st->rows = sel.n_rows;
    st->contigs = sel.cs.size();
    st->rows_selected = S;
    set_pair_stats(pc, pairs_paf != nullptr, st);

    // the spans: all that is read of the selected rows, and all that comes back of them for the layout
    DBuf<PolSpan> d_spans(std::max<size_t>(S, 1));
    depth_spans_from_rows(sel.rows.recs.p, sel.idx.p, S, sel.d_crec_of_rank.p, d_spans.p);
    const std::vector<PolSpan> spans = d_spans.download(S);
    for (const PolSpan &s : spans)
        if (s.contig >= sel.cs.size()) fail(HLMI_EINVAL, "hlmi_depth_reads: a row names a target that is no contig");      // (never)
    PolLayout L;
    polish_layout(sel.cs, spans, "hlmi_depth_reads", L, nullptr, false);
    DeviceDepth dev;
    if (S) {
        DBuf<PolTile> d_tiles;
        DBuf<uint32_t> d_cbase;
        d_tiles.upload(L.tiles);
        d_cbase.upload(L.cbase);
        DepthCoreIn in;
        in.spans = d_spans.p; in.n_spans = S;
        in.tiles = d_tiles.p; in.n_tiles = L.tiles.size();
        in.cbase = d_cbase.p; in.h_cbase = &L.cbase;
        in.want_runs = out_bedgraph != nullptr;
        depth_core(in, dev);
    }
    st->ms_device = now_ms() - sel.t_dev;
    depth_emit(sel.cs, L, dev, out_tsv, out_bedgraph, st);
    st->ms_total = now_ms() - t_begin;
}

}  // namespace hlmi
