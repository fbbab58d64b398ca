// variants_host.cpp - the host part of hlmi_variants, hlmi_variants_reads, their _ins forms and the _q forms of the four (include/hylight_mi.h): variant sites,
// insertion sites (_ins) and a summary per contig from the selected rows' votes.  The rows come from the pile-up calls' row front (polish_select.h: rows_from_paf or
// rows_from_reads), selected, laid out and in device memory; the votes, the site rule and the records are variants.hip's, the
// text variants_text.h's and variants_ins_text.h's.
// PARITY UNPINNED: a function of the project's own; tests/variants_model.py and tests/variants_ins_model.py are the contract.
#include <string>
#include <type_traits>
#include <string_view>
#include <vector>

#include "ava.h"
#include "common.h"
#include "paf_io.h"
#include "polish_internal.h"
#include "polish_select.h"
#include "variants_internal.h"
#include "variants_qual.h"

namespace hlmi {

using namespace pol;
using namespace var;

void var::check_variant_opts(const char *who, const hlmi_variant_opts &o) {
    if (o.min_cov < 1) fail(HLMI_EINVAL, "%s: min_cov %d (< 1)", who, o.min_cov);
    if (o.min_alt < 1) fail(HLMI_EINVAL, "%s: min_alt %d (< 1)", who, o.min_alt);
    if (!(o.min_frac >= 0.0 && o.min_frac <= 1.0)) fail(HLMI_EINVAL, "%s: min_frac %g (outside [0, 1] or not a number)", who, o.min_frac);
}

void var::check_variant_qfloors(const char *who, const hlmi_variant_qopts &q) {
    if (q.min_base_qual < 0 || q.min_base_qual > VQ_FLOOR_MAX) fail(HLMI_EINVAL, "%s: min_base_qual %d (outside 0..93)", who, q.min_base_qual);
    if (!(q.min_avg_qual >= 0.0)) fail(HLMI_EINVAL, "%s: min_avg_qual %g (negative or not a number)", who, q.min_avg_qual);
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

// what every entry point does behind the rows: the votes and the site rule, the records, the statistics and the files.  Stats is
// hlmi_variant_ins_stats for the _ins calls (out_ins is their file): one count pass with the slots' counters, the insertion
// sites' records, the third file and a summary of three columns more; out_sites and the thirteen shared fields are the same.
// qual != nullptr: a _q call - the base floor goes to the device part, and the three counters are set.
struct QualPart {
    int min_base_qual;
    const PolQualCall *front;           // reads_with_qual, rows_low_qual: the row front's
    hlmi_variant_qcounts *out;
};
template <class Stats>
void variants_body(const char *who, const PileupRows &R, const hlmi_variant_opts &o, const char *out_sites, const char *out_summary,
                   const char *out_ins, Stats *st, const QualPart *qual = nullptr) {
    constexpr bool INS = std::is_same_v<Stats, hlmi_variant_ins_stats>;
    const SeqSet &cs = R.cs();
    const PolLayout &L = R.L;
    set_row_stats(R, st);
    DeviceVariants dev;
    DeviceInsertions dins;
    if (qual) {
        uint64_t low = 0;
        if constexpr (INS) variants_ins_q_core(R.up.core, o, qual->min_base_qual, dev, dins, low);
        else variants_q_core(R.up.core, o, qual->min_base_qual, dev, low);
        *qual->out = hlmi_variant_qcounts{qual->front->reads_with_qual, qual->front->rows_low_qual, low};
    } else if constexpr (INS) variants_ins_core(R.up.core, o, dev, dins);
    else variants_core(R.up.core, o, dev);
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
    std::vector<std::string> summary, ins;
    if constexpr (INS) {
        InsTotals itot;
        const std::vector<ContigInsertions> irecs = contig_insertions(L.rc, L.slot_of_contig, dins, &itot);
        if (!ins_lines(cs.names, seq, L.rc, L.slot_of_contig, L.cbase, dins, ins) || itot.ins_sites != dins.recs.size())
            fail(HLMI_ESTATE, "%s: the insertion sites' records do not fit the contigs", who);                      // (never)
        st->slots_callable = itot.slots_callable;
        st->ins_sites = itot.ins_sites;
        st->ins_long = R.ins_long;
        st->ins_edge = R.ins_edge;
        stat_set("variants_ins_slot_sites", (double)dins.slot_sites);
        if (out_summary) summary = ins_summary_lines(recs, irecs);
    } else if (out_summary)
        summary = summary_lines(recs);
    write_lines(out_sites, sites);
    if constexpr (INS) write_lines(out_ins, ins);
    if (out_summary) write_lines(out_summary, summary);
}

// the two kinds of rows in front of the body; who: the entry point's name in every refusal
template <class Stats>
void run_paf(const char *who, const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts &o, const char *pairs_paf,
             const char *out_sites, const char *out_summary, const char *out_ins, Stats *st) {
    timed_call(st, true, [&] {
        check_variant_opts(who, o);
        PileupRows R;
        rows_from_paf(contigs, reads, paf, plain_request(who, o.min_len, o.min_iden, pairs_paf), R);
        variants_body(who, R, o, out_sites, out_summary, out_ins, st);
    });
}
template <class Stats>
void run_reads(const char *who, const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_opts &o,
               const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins, Stats *st) {
    timed_call(st, true, [&] {
        check_variant_opts(who, o);
        PileupRows R;
        rows_from_reads(contigs, reads, ao, plain_request(who, o.min_len, o.min_iden, pairs_paf), R);
        variants_body(who, R, o, out_sites, out_summary, out_ins, st);
    });
}

// The _q calls.  Refusals: the two floors before anything is read, then out_ins == NULL (capi.cpp hands it on for that), then the
// older call's in its order.  The request: the front's _q part with the read floor and no weights (polish_check_weight_width
// stays quiet: the counters hold counts); with a base floor the quality bytes travel, FASTA records as a passing byte.
hlmi_variant_opts check_variant_qopts(const char *who, const hlmi_variant_qopts &q, bool ins, const char *out_ins) {
    check_variant_qfloors(who, q);
    if (ins && !out_ins) fail(HLMI_EINVAL, "%s: out_ins is NULL", who);
    const hlmi_variant_opts o{q.min_len, q.min_iden, q.min_cov, q.min_alt, q.min_frac};
    check_variant_opts(who, o);
    return o;
}
RowsRequest qual_request(const char *who, const hlmi_variant_qopts &q, const char *pairs_paf, PolQualCall *front) {
    *front = PolQualCall{0, q.min_avg_qual};
    RowsRequest r = plain_request(who, q.min_len, q.min_iden, pairs_paf);
    r.qc = front;
    r.quals_fill = q.min_base_qual > 0 ? VQ_FASTA_FILL : 0;
    return r;
}
template <class Stats>
void run_q(const char *who, const char *contigs, const char *reads, const char *paf, const hlmi_ava_opts *ao, const hlmi_variant_qopts &q,
           const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins, Stats *st,
           hlmi_variant_qcounts *qc) {
    *qc = hlmi_variant_qcounts{};
    timed_call(st, true, [&] {
        const hlmi_variant_opts o = check_variant_qopts(who, q, std::is_same_v<Stats, hlmi_variant_ins_stats>, out_ins);
        PileupRows R;
        PolQualCall front;
        const RowsRequest req = qual_request(who, q, pairs_paf, &front);
        if (ao) rows_from_reads(contigs, reads, *ao, req, R);
        else rows_from_paf(contigs, reads, paf, req, R);
        const QualPart part{q.min_base_qual, &front, qc};
        variants_body(who, R, o, out_sites, out_summary, out_ins, st, &part);
    });
}

}  // namespace

void variants_q_run(const char *contigs, const char *reads, const char *paf, const hlmi_variant_qopts &q, const char *pairs_paf,
                    const char *out_sites, const char *out_summary, hlmi_variant_stats *st, hlmi_variant_qcounts *qc) {
    run_q("hlmi_variants_q", contigs, reads, paf, nullptr, q, pairs_paf, out_sites, out_summary, nullptr, st, qc);
}

void variants_reads_q_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_qopts &q,
                          const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st,
                          hlmi_variant_qcounts *qc) {
    run_q("hlmi_variants_reads_q", contigs, reads, nullptr, &ao, q, pairs_paf, out_sites, out_summary, nullptr, st, qc);
}

void variants_ins_q_run(const char *contigs, const char *reads, const char *paf, const hlmi_variant_qopts &q, const char *pairs_paf,
                        const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st,
                        hlmi_variant_qcounts *qc) {
    run_q("hlmi_variants_ins_q", contigs, reads, paf, nullptr, q, pairs_paf, out_sites, out_summary, out_ins, st, qc);
}

void variants_reads_ins_q_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_qopts &q,
                              const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins,
                              hlmi_variant_ins_stats *st, hlmi_variant_qcounts *qc) {
    run_q("hlmi_variants_reads_ins_q", contigs, reads, nullptr, &ao, q, pairs_paf, out_sites, out_summary, out_ins, st, qc);
}

void variants_run(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts &o, const char *pairs_paf,
                  const char *out_sites, const char *out_summary, hlmi_variant_stats *st) {
    run_paf("hlmi_variants", contigs, reads, paf, o, pairs_paf, out_sites, out_summary, nullptr, st);
}

void variants_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_opts &o,
                        const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st) {
    run_reads("hlmi_variants_reads", contigs, reads, ao, o, pairs_paf, out_sites, out_summary, nullptr, st);
}

void variants_ins_run(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts &o, const char *pairs_paf,
                      const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st) {
    run_paf("hlmi_variants_ins", contigs, reads, paf, o, pairs_paf, out_sites, out_summary, out_ins, st);
}

void variants_reads_ins_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_opts &o,
                            const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins,
                            hlmi_variant_ins_stats *st) {
    run_reads("hlmi_variants_reads_ins", contigs, reads, ao, o, pairs_paf, out_sites, out_summary, out_ins, st);
}

}  // namespace hlmi
