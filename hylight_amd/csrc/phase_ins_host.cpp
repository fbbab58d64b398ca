// phase_ins_host.cpp - the host part of hlmi_phase_ins and hlmi_phase_reads_ins (include/hylight_mi.h): hlmi_phase_reach over the
// merged list of hlmi_variants's position sites and the insertion sites of hlmi_variants_ins that take part.  The rows come from the
// pile-up calls' row front (polish_select.h); both kinds of sites from the one count pass (variants_ins_core); the merge, the
// takes-part rule and the lines with their `+` marks are phase_ins_text.h's, the allele table phase_ins.hip's, everything behind
// it phase.hip's tail.  The shared statistics are phase_emit's, asked for without a file.
// PARITY UNPINNED: a function of the project's own; tests/phase_ins_model.py is the contract.
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

// what both entry points do behind the rows
void phase_ins_body(const char *who, const PileupRows &R, const hlmi_phase_opts &o, int reach, const char *out_sites, const char *out_links,
                    const char *out_reads, hlmi_phase_ins_stats *st) {
    const SeqSet &cs = R.cs();
    const PolLayout &L = R.L;
    hlmi_phase_stats *base = &st->reach.base;
    set_row_stats(R, base);
    Phased P;
    DeviceInsertions dins;
    variants_ins_core(R.up.core, hlmi_variant_opts{o.min_len, o.min_iden, o.min_cov, o.min_alt, o.min_frac}, P.var, dins);
    std::vector<uint64_t> length;
    std::vector<std::string_view> seq;
    contig_views(cs, length, seq);
    MergedSites M;
    std::vector<std::string> unused;
    InsTotals itot;
    contig_insertions(L.rc, L.slot_of_contig, dins, &itot);
    if (!phase_sites(seq, L.rc, L.slot_of_contig, L.cbase, P.var, P.sites) ||
        !ins_lines(cs.names, seq, L.rc, L.slot_of_contig, L.cbase, dins, unused) || itot.ins_sites != dins.recs.size() ||
        !merge_sites(seq, L.rc, L.slot_of_contig, L.cbase, P.sites, dins, o.min_alt, M))
        fail(HLMI_ESTATE, "%s: the sites' records do not fit the contigs", who);                                    // (never)
    phase_ins_core(who, R.up.core, M, o, P.dev, reach);
    std::vector<uint32_t> rows_read;            // when a record needs its read's name (aligned rows: 4 bytes per row come down)
    if (out_reads && !P.dev.recs.empty()) rows_read = R.read_of_row();
    base->ms_device = now_ms() - R.t_dev;

    // the statistics hlmi_phase_reach has, by its code: P.sites are the position sites, P.dev counts over the merged list
    phase_emit(who, R, P, o, {}, nullptr, nullptr, nullptr, base, &st->reach);
    st->slots_callable = itot.slots_callable;
    st->ins_sites = itot.ins_sites;
    st->ins_long = R.ins_long;
    st->ins_edge = R.ins_edge;
    st->ins_sites_phasing = M.ins_sites_phasing;
    st->ins_sites_left_out = M.ins_sites_left_out;
    const Blocks &B = P.dev.blocks;
    st->ins_sites_phased = ins_sites_phased(M, B);
    stat_set("variants_ins_slot_sites", (double)dins.slot_sites);

    std::vector<std::string> sites, links, reads;
    sites = phase_ins_site_lines(cs.names, M, B);
    if (out_links) links = phase_ins_link_lines(cs.names, M, P.dev.far, o.min_link, o.min_agree);
    if (out_reads && !phase_ins_read_lines(cs.names, R.rs().names, rows_read, M, B, P.dev.recs, &reads, nullptr))
        fail(HLMI_ESTATE, "%s: a row's record names no block or no read", who);                                     // (never)
    write_lines(out_sites, sites);
    if (out_links) write_lines(out_links, links);
    if (out_reads) write_lines(out_reads, reads);
}

}  // namespace

void phase_ins_run(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts &o, int reach, const char *pairs_paf,
                   const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_ins_stats *st) {
    *st = hlmi_phase_ins_stats{};
    timed_call(&st->reach.base, true, [&] {
        check_phase_opts("hlmi_phase_ins", o);
        check_reach("hlmi_phase_ins", reach);
        PileupRows R;
        rows_from_paf(contigs, reads, paf, plain_request("hlmi_phase_ins", o.min_len, o.min_iden, pairs_paf), R);
        phase_ins_body("hlmi_phase_ins", R, o, reach, out_sites, out_links, out_reads, st);
    });
}

void phase_reads_ins_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_phase_opts &o, int reach,
                         const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads,
                         hlmi_phase_ins_stats *st) {
    *st = hlmi_phase_ins_stats{};
    timed_call(&st->reach.base, true, [&] {
        check_phase_opts("hlmi_phase_reads_ins", o);
        check_reach("hlmi_phase_reads_ins", reach);
        PileupRows R;
        rows_from_reads(contigs, reads, ao, plain_request("hlmi_phase_reads_ins", o.min_len, o.min_iden, pairs_paf), R);
        phase_ins_body("hlmi_phase_reads_ins", R, o, reach, out_sites, out_links, out_reads, st);
    });
}

}  // namespace hlmi
