// variants_host.cpp - the host part of hlmi_variants and hlmi_variants_reads (include/hylight_mi.h): variant sites and a summary
// per contig from the selected rows' votes.  The rows come from the pile-up calls' row front (polish_select.h: rows_from_paf or
// rows_from_reads), selected, laid out and in device memory; the votes, the site rule and the records are variants.hip's, the
// text variants_text.h's.
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

void var::contig_views(const SeqSet &cs, std::vector<uint64_t> &length, std::vector<std::string_view> &seq) {
    length.resize(cs.size());
    seq.resize(cs.size());
    for (size_t c = 0; c < cs.size(); ++c) {
        length[c] = cs.len(c);
        seq[c] = std::string_view(cs.bases).substr(cs.off[c], cs.len(c));
    }
}

namespace {

// what both entry points do behind the rows: the votes and the site rule, the records, the statistics and the two files
void variants_body(const char *who, const PileupRows &R, const hlmi_variant_opts &o, const char *out_sites, const char *out_summary,
                   hlmi_variant_stats *st) {
    const SeqSet &cs = R.cs();
    const PolLayout &L = R.L;
    set_row_stats(R, st);
    DeviceVariants dev;
    variants_core(R.up.core, o, dev);
    st->ms_device = now_ms() - R.t_dev;

    std::vector<uint64_t> length;
    std::vector<std::string_view> seq;
    contig_views(cs, length, seq);
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

}  // namespace

void variants_run(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts &o, const char *pairs_paf,
                  const char *out_sites, const char *out_summary, hlmi_variant_stats *st) {
    timed_call(st, true, [&] {
        check_variant_opts("hlmi_variants", o);
        PileupRows R;
        rows_from_paf(contigs, reads, paf, plain_request("hlmi_variants", o.min_len, o.min_iden, pairs_paf), R);
        variants_body("hlmi_variants", R, o, out_sites, out_summary, st);
    });
}

void variants_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_opts &o,
                        const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st) {
    timed_call(st, true, [&] {
        check_variant_opts("hlmi_variants_reads", o);
        PileupRows R;
        rows_from_reads(contigs, reads, ao, plain_request("hlmi_variants_reads", o.min_len, o.min_iden, pairs_paf), R);
        variants_body("hlmi_variants_reads", R, o, out_sites, out_summary, st);
    });
}

}  // namespace hlmi
