// phase_host.cpp - the host part of hlmi_phase and hlmi_phase_reads (include/hylight_mi.h): the variant sites of hlmi_variants
// phased from the reads - links between neighbouring sites, blocks, and every read's side per block.  The rows come from the
// pile-up calls' row front (polish_select.h), the sites are variants_core's over them; the allele table, the link counters and the
// records per (row, block) are phase.hip's, the rules' arithmetic and the three files' text phase_text.h's.  phase_device and
// phase_emit are the two halves of the body that hlmi_haplotigs calls as well.  hlmi_phase_reach and hlmi_phase_reads_reach are
// the same four statements with `reach` handed down: links of every distance up to it (phase_reach.hip), the block rule and the
// two files that differ in phase_reach_text.h.
// PARITY UNPINNED: a function of the project's own; tests/phase_model.py and tests/phase_reach_model.py are the contract.
#include <cmath>
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

void check_reach(const char *who, int reach) {
    if (reach < 1 || reach > HLMI_PHASE_REACH_MAX) fail(HLMI_EINVAL, "%s: reach %d (outside [1, %d])", who, reach, HLMI_PHASE_REACH_MAX);
}

void phase_device(const char *who, const PileupRows &R, const hlmi_phase_opts &o, Phased &P, DevRecs *keep, int reach) {
    const SeqSet &cs = R.cs();
    const PolLayout &L = R.L;
    variants_core(R.up.core, variant_part(o), P.var);
    std::vector<std::string_view> seq(cs.size());
    for (size_t c = 0; c < cs.size(); ++c) seq[c] = std::string_view(cs.bases).substr(cs.off[c], cs.len(c));
    if (!phase_sites(seq, L.rc, L.slot_of_contig, L.cbase, P.var, P.sites))
        fail(HLMI_ESTATE, "%s: the sites' records do not fit the contigs", who);                                    // (never)
    phase_core(who, R.up.core, P.sites, o, P.dev, keep, reach);
}

void phase_emit(const char *who, const PileupRows &R, const Phased &P, const hlmi_phase_opts &o, const std::vector<uint32_t> &rows_read,
                const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st, hlmi_phase_reach_stats *far) {
    const SeqSet &cs = R.cs();
    const PolLayout &L = R.L;
    const bool reach = P.dev.far.reach >= 1;
    std::vector<uint64_t> length;
    std::vector<std::string_view> seq;
    contig_views(cs, length, seq);
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
    if (far) {
        far->links_far = P.dev.links_far;
        far->links_far_phased = P.dev.links_far_phased;
        far->joins_far = P.dev.joins_far;
        far->sites_bridged = P.dev.sites_bridged;
        far->links_conflict = P.dev.links_conflict;
    }
    stat_set("variants_tiles", (double)P.var.tiles);
    stat_set("variants_tiles_revisited", (double)P.var.tiles_revisited);

    std::vector<std::string> sites, links, reads;
    if (out_sites) sites = reach ? phase_reach_site_lines(cs.names, P.sites, B) : phase_site_lines(cs.names, P.sites, B);
    if (out_links)
        links = reach ? phase_reach_link_lines(cs.names, P.sites, P.dev.far, o.min_link, o.min_agree)
                      : phase_link_lines(cs.names, P.sites, P.dev.links, o.min_link, o.min_agree);
    ReadTotals rt;
    if (!phase_read_lines(cs.names, R.rs().names, rows_read, P.sites, B, P.dev.recs, out_reads ? &reads : nullptr, &rt))
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

namespace {

// what the entry points do behind the rows: sites and phasing, the statistics and the three files.  reach 0: the plain calls
void phase_body(const char *who, const PileupRows &R, const hlmi_phase_opts &o, const char *out_sites, const char *out_links,
                const char *out_reads, hlmi_phase_stats *st, int reach = 0, hlmi_phase_reach_stats *far = nullptr) {
    set_row_stats(R, st);
    Phased P;
    phase_device(who, R, o, P, nullptr, reach);
    std::vector<uint32_t> rows_read;            // when a record needs its read's name (aligned rows: 4 bytes per row come down)
    if (out_reads && !P.dev.recs.empty()) rows_read = R.read_of_row();
    st->ms_device = now_ms() - R.t_dev;
    phase_emit(who, R, P, o, rows_read, out_sites, out_links, out_reads, st, far);
}

}  // namespace

void phase_run(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts &o, const char *pairs_paf,
               const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st) {
    timed_call(st, true, [&] {
        check_phase_opts("hlmi_phase", o);
        PileupRows R;
        rows_from_paf(contigs, reads, paf, plain_request("hlmi_phase", o.min_len, o.min_iden, pairs_paf), R);
        phase_body("hlmi_phase", R, o, out_sites, out_links, out_reads, st);
    });
}

void phase_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_phase_opts &o, const char *pairs_paf,
                     const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st) {
    timed_call(st, true, [&] {
        check_phase_opts("hlmi_phase_reads", o);
        PileupRows R;
        rows_from_reads(contigs, reads, ao, plain_request("hlmi_phase_reads", o.min_len, o.min_iden, pairs_paf), R);
        phase_body("hlmi_phase_reads", R, o, out_sites, out_links, out_reads, st);
    });
}

void phase_reach_run(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts &o, int reach, const char *pairs_paf,
                     const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_reach_stats *st) {
    *st = hlmi_phase_reach_stats{};
    timed_call(&st->base, true, [&] {
        check_phase_opts("hlmi_phase_reach", o);
        check_reach("hlmi_phase_reach", reach);
        PileupRows R;
        rows_from_paf(contigs, reads, paf, plain_request("hlmi_phase_reach", o.min_len, o.min_iden, pairs_paf), R);
        phase_body("hlmi_phase_reach", R, o, out_sites, out_links, out_reads, &st->base, reach, st);
    });
}

void phase_reads_reach_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_phase_opts &o, int reach,
                           const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads,
                           hlmi_phase_reach_stats *st) {
    *st = hlmi_phase_reach_stats{};
    timed_call(&st->base, true, [&] {
        check_phase_opts("hlmi_phase_reads_reach", o);
        check_reach("hlmi_phase_reads_reach", reach);
        PileupRows R;
        rows_from_reads(contigs, reads, ao, plain_request("hlmi_phase_reads_reach", o.min_len, o.min_iden, pairs_paf), R);
        phase_body("hlmi_phase_reads_reach", R, o, out_sites, out_links, out_reads, &st->base, reach, st);
    });
}

}  // namespace hlmi
