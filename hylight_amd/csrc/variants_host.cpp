// variants_host.cpp - the host part of hlmi_variants and hlmi_variants_reads (include/hylight_mi.h): variant sites and a summary
// per contig from the selected rows' votes.  The selection is the polisher's own (polish_select.h), and so are the layout of the
// covered contigs and their tiles (polish_layout) and the rows, compact CIGARs and reads the device works on (paf_rows_input /
// device_rows_input); the votes, the site rule and the records are variants.hip's, the text variants_text.h's.
// PARITY UNPINNED: a function of the project's own; tests/variants_model.py is the contract.
#include <string>
#include <string_view>
#include <vector>

#include "ava.h"
#include "common.h"
#include "paf_io.h"
#include "polish_internal.h"
#include "polish_select.h"
#include "variants_internal.h"

namespace hlmi {

using namespace pol;
using namespace var;

void var::check_variant_opts(const char *who, const hlmi_variant_opts &o) {
    if (o.min_cov < 1) fail(HLMI_EINVAL, "%s: min_cov %d (< 1)", who, o.min_cov);
    if (o.min_alt < 1) fail(HLMI_EINVAL, "%s: min_alt %d (< 1)", who, o.min_alt);
    if (!(o.min_frac >= 0.0 && o.min_frac <= 1.0)) fail(HLMI_EINVAL, "%s: min_frac %g (outside [0, 1] or not a number)", who, o.min_frac);
}

namespace {

// what both entry points do behind the device part: the records, the statistics and the two files
void variants_emit(const char *who, const SeqSet &cs, const PolLayout &L, const DeviceVariants &dev, const char *out_sites,
                   const char *out_summary, hlmi_variant_stats *st) {
    std::vector<uint64_t> length(cs.size());
    std::vector<std::string_view> seq(cs.size());
    for (size_t c = 0; c < cs.size(); ++c) {
        length[c] = cs.len(c);
        seq[c] = std::string_view(cs.bases).substr(cs.off[c], cs.len(c));
    }
    VariantTotals tot;
    const std::vector<ContigVariants> recs = contig_records(cs.names, length, L.rc, L.slot_of_contig, dev, &tot);
    std::vector<std::string> sites;
    if (!site_lines(cs.names, seq, L.rc, L.slot_of_contig, L.cbase, dev, sites, &tot) || tot.sites != dev.recs.size())
        fail(HLMI_ESTATE, "%s: the sites' records do not fit the contigs", who);                                    // (never)
    st->contigs_covered = tot.contigs_covered;
    st->positions = tot.positions;
    st->callable = tot.callable;
    st->ref_other = tot.ref_other;
    st->sites = tot.sites;
    st->sites_base = tot.sites_base;
    st->sites_del = tot.sites_del;
    stat_set("variants_tiles", (double)dev.tiles);
    stat_set("variants_tiles_revisited", (double)dev.tiles_revisited);
    std::vector<std::string> summary;
    if (out_summary) summary = summary_lines(recs);
    write_lines(out_sites, sites);
    if (out_summary) write_lines(out_summary, summary);
}

void set_pair_stats(const PolPairCall &pc, bool given, hlmi_variant_stats *st) {
    if (!given) return;
    st->pairs_listed = pc.pairs_listed;
    st->pairs_unknown = pc.pairs_unknown;
    st->rows_not_listed = pc.rows_not_listed;
}

}  // namespace

void variants_run(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts &o, const char *pairs_paf,
                  const char *out_sites, const char *out_summary, hlmi_variant_stats *st) {
    const double t_begin = now_ms();
    *st = hlmi_variant_stats{};
    stat_reset();
    check_variant_opts("hlmi_variants", o);
    PolQualCall qc;                             // no floor and no weights: the quality strings are only checked, as hlmi_depth does
    PolPairCall pc;
    pc.path = pairs_paf;
    PafSelection S;
    select_paf_rows(contigs, reads, paf, o.min_len, o.min_iden, SelectNames{"hlmi_variants", "hlmi_variants", "hlmi_variants", true}, &qc,
                    pairs_paf ? &pc : nullptr, S);
    st->rows = S.pt.recs.size();
    st->contigs = S.cs.size();
    st->rows_selected = S.sel.size();
    set_pair_stats(pc, pairs_paf != nullptr, st);
    std::vector<PolSpan> spans;
    spans.reserve(S.sel.size());
    for (const PafSel &s : S.sel) spans.push_back(PolSpan{s.contig, S.pt.recs[s.line].ts, S.pt.recs[s.line].te});
    PolLayout L;
    polish_layout(S.cs, spans, "hlmi_variants", L, nullptr);
    PolDevIn in;
    uint64_t ins_edge = 0, ins_long = 0;        // insertions take no part
    paf_rows_input(S, L, false, in, ins_edge, ins_long);
    in.contigs = std::move(L.contigs);
    in.cbase = L.cbase;
    in.tiles = std::move(L.tiles);

    const double t_dev = now_ms();
    DeviceVariants dev;
    {
        PolUploaded up;
        polish_upload(in, up);
        variants_core(up.core, o, dev);
    }
    st->ms_device = now_ms() - t_dev;
    variants_emit("hlmi_variants", S.cs, L, dev, out_sites, out_summary, st);
    st->ms_total = now_ms() - t_begin;
}

void variants_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_opts &o,
                        const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st) {
    const double t_begin = now_ms();
    *st = hlmi_variant_stats{};
    stat_reset();
    check_variant_opts("hlmi_variants_reads", o);
    PolPairCall pc;
    pc.path = pairs_paf;
    RowSelection sel;
    select_device_rows(contigs, reads, ao, o.min_len, o.min_iden,
                       SelectNames{"hlmi_variants_reads", "hlmi_variants_reads", "hlmi_variants_reads", true}, nullptr,
                       pairs_paf ? &pc : nullptr, sel);
    st->rows = sel.n_rows;
    st->contigs = sel.cs.size();
    st->rows_selected = sel.n_sel;
    set_pair_stats(pc, pairs_paf != nullptr, st);
    DeviceRowsInput in;
    device_rows_input(sel, "hlmi_variants_reads", false, nullptr, in);
    DeviceVariants dev;
    variants_core(in.core, o, dev);
    st->ms_device = now_ms() - sel.t_dev;
    variants_emit("hlmi_variants_reads", sel.cs, in.L, dev, out_sites, out_summary, st);
    st->ms_total = now_ms() - t_begin;
}

}  // namespace hlmi
