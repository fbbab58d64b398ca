// phase_host.cpp - the host part of hlmi_phase and hlmi_phase_reads (include/hylight_mi.h): the variant sites of hlmi_variants
// phased from the reads - links between neighbouring sites, blocks, and every read's side per block.  Selection, layout, rows,
// compact CIGARs and reads are the polisher's (polish_select.h), the sites variants_core's, exactly as variants_host.cpp reaches
// them; the allele table, the link counters and the records per (row, block) are phase.hip's, the rules' arithmetic and the
// three files' text phase_text.h's.
// PARITY UNPINNED: a function of the project's own; tests/phase_model.py is the contract.
#include <cmath>
#include <functional>
#include <string>
#include <string_view>
#include <vector>

#include "ava.h"
#include "common.h"
#include "paf_io.h"
#include "phase_internal.h"
#include "polish_internal.h"
#include "polish_select.h"
#include "variants_internal.h"

namespace hlmi {

using namespace pol;
using namespace var;
using namespace ph;

namespace {

hlmi_variant_opts variant_part(const hlmi_phase_opts &o) { return hlmi_variant_opts{o.min_len, o.min_iden, o.min_cov, o.min_alt, o.min_frac}; }

}  // namespace

namespace ph {

void check_phase_opts(const char *who, const hlmi_phase_opts &o) {
    check_variant_opts(who, variant_part(o));
    if (o.min_link < 1) fail(HLMI_EINVAL, "%s: min_link %d (< 1)", who, o.min_link);
    if (!(o.min_agree > 0.5 && o.min_agree <= 1.0)) fail(HLMI_EINVAL, "%s: min_agree %g (outside (0.5, 1] or not a number)", who, o.min_agree);
}

void set_pair_stats(const PolPairCall &pc, bool given, hlmi_phase_stats *st) {
    if (!given) return;
    st->pairs_listed = pc.pairs_listed;
    st->pairs_unknown = pc.pairs_unknown;
    st->rows_not_listed = pc.rows_not_listed;
}

void phase_device(const char *who, const SeqSet &cs, const PolLayout &L, const PolCoreIn &core, const hlmi_phase_opts &o, Phased &P,
                  DevRecs *keep) {
    variants_core(core, variant_part(o), P.var);
    std::vector<std::string_view> seq(cs.size());
    for (size_t c = 0; c < cs.size(); ++c) seq[c] = std::string_view(cs.bases).substr(cs.off[c], cs.len(c));
    if (!phase_sites(seq, L.rc, L.slot_of_contig, L.cbase, P.var, P.sites))
        fail(HLMI_ESTATE, "%s: the sites' records do not fit the contigs", who);                                    // (never)
    phase_core(who, core, P.sites, o, P.dev, keep);
}

void phase_emit(const char *who, const SeqSet &cs, const SeqSet &rs, const PolLayout &L, const Phased &P, const hlmi_phase_opts &o,
                const std::function<std::vector<uint32_t>()> &read_of_row, const char *out_sites, const char *out_links,
                const char *out_reads, hlmi_phase_stats *st) {
    std::vector<uint64_t> length(cs.size());
    std::vector<std::string_view> seq(cs.size());
    for (size_t c = 0; c < cs.size(); ++c) {
        length[c] = cs.len(c);
        seq[c] = std::string_view(cs.bases).substr(cs.off[c], cs.len(c));
    }
    VariantTotals tot;                          // the shared stats, by the code hlmi_variants counts them with
    contig_records(cs.names, length, L.rc, L.slot_of_contig, P.var, &tot);
    std::vector<std::string> unused;
    if (!site_lines(cs.names, seq, L.rc, L.slot_of_contig, L.cbase, P.var, unused, &tot) || tot.sites != P.sites.size())
        fail(HLMI_ESTATE, "%s: the sites' records do not fit the contigs", who);                                    // (never)
    st->contigs_covered = tot.contigs_covered;
    st->positions = tot.positions;
    st->callable = tot.callable;
    st->ref_other = tot.ref_other;
    st->sites = tot.sites;
    st->sites_base = tot.sites_base;
    st->sites_del = tot.sites_del;
    const Blocks &B = P.dev.blocks;
    st->links = B.links;
    st->links_phased = B.links_phased;
    st->blocks = B.first.size();
    st->blocks_multi = B.blocks_multi;
    st->sites_phased = B.sites_phased;
    st->alleles = P.dev.alleles;
    stat_set("variants_tiles", (double)P.var.tiles);
    stat_set("variants_tiles_revisited", (double)P.var.tiles_revisited);

    std::vector<std::string> sites, links, reads;
    if (out_sites) sites = phase_site_lines(cs.names, P.sites, B);
    if (out_links) links = phase_link_lines(cs.names, P.sites, P.dev.links, o.min_link, o.min_agree);
    ReadTotals rt;
    std::vector<uint32_t> rows_read;
    if (out_reads && !P.dev.recs.empty()) rows_read = read_of_row();
    if (!phase_read_lines(cs.names, rs.names, rows_read, P.sites, B, P.dev.recs, out_reads ? &reads : nullptr, &rt))
        fail(HLMI_ESTATE, "%s: a row's record names no block or no read", who);                                     // (never)
    st->read_records = rt.records;
    st->reads_a = rt.a;
    st->reads_b = rt.b;
    st->reads_tie = rt.tie;
    if (out_sites) write_lines(out_sites, sites);
    if (out_links) write_lines(out_links, links);
    if (out_reads) write_lines(out_reads, reads);
}

}  // namespace ph

void phase_run(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts &o, const char *pairs_paf,
               const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st) {
    const double t_begin = now_ms();
    *st = hlmi_phase_stats{};
    stat_reset();
    check_phase_opts("hlmi_phase", o);
    PolQualCall qc;                             // no floor and no weights: the quality strings are only checked, as hlmi_variants does
    PolPairCall pc;
    pc.path = pairs_paf;
    PafSelection S;
    select_paf_rows(contigs, reads, paf, o.min_len, o.min_iden, SelectNames{"hlmi_phase", "hlmi_phase", "hlmi_phase", true}, &qc,
                    pairs_paf ? &pc : nullptr, S);
    st->rows = S.pt.recs.size();
    st->contigs = S.cs.size();
    st->rows_selected = S.sel.size();
    set_pair_stats(pc, pairs_paf != nullptr, st);
    std::vector<PolSpan> spans;
    spans.reserve(S.sel.size());
    for (const PafSel &s : S.sel) spans.push_back(PolSpan{s.contig, S.pt.recs[s.line].ts, S.pt.recs[s.line].te});
    PolLayout L;
    polish_layout(S.cs, spans, "hlmi_phase", L, nullptr);
    PolDevIn in;
    uint64_t ins_edge = 0, ins_long = 0;        // insertions take no part
    paf_rows_input(S, L, false, in, ins_edge, ins_long);
    in.contigs = std::move(L.contigs);
    in.cbase = L.cbase;
    in.tiles = std::move(L.tiles);

    const double t_dev = now_ms();
    Phased P;
    {
        PolUploaded up;
        polish_upload(in, up);
        phase_device("hlmi_phase", S.cs, L, up.core, o, P);
    }
    st->ms_device = now_ms() - t_dev;
    phase_emit("hlmi_phase", S.cs, S.rs, L, P, o, [&]() {
        std::vector<uint32_t> r(S.sel.size());
        for (size_t i = 0; i < S.sel.size(); ++i) r[i] = S.sel[i].read;
        return r;
    }, out_sites, out_links, out_reads, st);
    st->ms_total = now_ms() - t_begin;
}

void phase_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_phase_opts &o, const char *pairs_paf,
                     const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st) {
    const double t_begin = now_ms();
    *st = hlmi_phase_stats{};
    stat_reset();
    check_phase_opts("hlmi_phase_reads", o);
    PolPairCall pc;
    pc.path = pairs_paf;
    RowSelection sel;
    select_device_rows(contigs, reads, ao, o.min_len, o.min_iden, SelectNames{"hlmi_phase_reads", "hlmi_phase_reads", "hlmi_phase_reads", true},
                       nullptr, pairs_paf ? &pc : nullptr, sel);
    st->rows = sel.n_rows;
    st->contigs = sel.cs.size();
    st->rows_selected = sel.n_sel;
    set_pair_stats(pc, pairs_paf != nullptr, st);
    DeviceRowsInput in;
    device_rows_input(sel, "hlmi_phase_reads", false, nullptr, in);
    Phased P;
    phase_device("hlmi_phase_reads", sel.cs, in.L, in.core, o, P);
    std::vector<uint32_t> rows_read;            // 4 bytes per selected row, when a record needs its read's name
    if (out_reads && !P.dev.recs.empty()) {
        rows_read = selected_query_ranks(sel.rows.recs.p, sel.idx.p, sel.n_sel);
        for (uint32_t &q : rows_read) q = q < sel.qrec_of_rank.size() ? sel.qrec_of_rank[q] : 0xffffffffu;
    }
    st->ms_device = now_ms() - sel.t_dev;
    phase_emit("hlmi_phase_reads", sel.cs, sel.rs, in.L, P, o, [&]() { return rows_read; }, out_sites, out_links, out_reads, st);
    st->ms_total = now_ms() - t_begin;
}

}  // namespace hlmi
