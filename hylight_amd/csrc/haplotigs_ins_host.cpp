// haplotigs_ins_host.cpp - the host part of hlmi_haplotigs_ins and hlmi_haplotigs_reads_ins (include/hylight_mi.h): the contigs
// polished once per side of every split block of hlmi_phase_ins's phasing, whose blocks may begin or end at an insertion site.
// The rows come from the pile-up calls' row front (polish_select.h); both kinds of sites, the merged list and the phasing are
// hlmi_phase_ins's, by its code (variants_ins_core, merge_sites, phase_ins_core, phase_emit for the shared statistics); the split
// rule and the records are haplotigs_host.cpp's (haplotig_blocks, haplotig_records); extents in key space, diff_slots and the
// ten-column blocks file are haplotigs_ins_text.h's, the key-space instantiations of the kernels haplotigs.hip's.  With no split
// block the single-sided polish_core gives the bytes and no kernel of haplotigs.hip runs.
// PARITY UNPINNED: a function of the project's own; tests/haplotigs_ins_model.py is the contract.
#include <string>
#include <string_view>
#include <vector>

#include "ava.h"
#include "common.h"
#include "haplotigs_ins_text.h"
#include "haplotigs_internal.h"
#include "paf_io.h"
#include "phase_internal.h"
#include "polish_internal.h"
#include "polish_select.h"
#include "variants_internal.h"

namespace hlmi {

using namespace pol;
using namespace var;
using namespace ph;
using namespace hap;

namespace {

// what both entry points do behind the rows
void haplotigs_ins_body(const char *who, PileupRows &R, const hlmi_haplotig_opts &o, int reach, const char *out_fa, const char *out_blocks,
                        hlmi_haplotig_ins_stats *st) {
    const SeqSet &cs = R.cs();
    const PolLayout &L = R.L;
    const double t_dev = R.t_dev;
    const hlmi_phase_opts po = phase_part(o);
    hlmi_haplotig_stats *base = &st->base;
    set_row_stats(R, &base->phase);
    base->ins_edge = R.ins_edge;
    base->ins_long = R.ins_long;
    PolCoreIn &core = R.up.core;
    core.min_cov = o.min_cov;
    core.quals = nullptr;
    Phased P;
    DeviceInsertions dins;
    MergedSites M;
    InsTotals itot;
    std::vector<KBlock> kb;
    PolDevOut out;
    bool any = false;
    {
        DevRecs keep;
        variants_ins_core(core, hlmi_variant_opts{o.min_len, o.min_iden, o.min_cov, o.min_alt, o.min_frac}, P.var, dins);
        std::vector<uint64_t> length;
        std::vector<std::string_view> seq;
        contig_views(cs, length, seq);
        std::vector<std::string> unused;
        contig_insertions(L.rc, L.slot_of_contig, dins, &itot);
        if (!phase_sites(seq, L.rc, L.slot_of_contig, L.cbase, P.var, P.sites) ||
            !ins_lines(cs.names, seq, L.rc, L.slot_of_contig, L.cbase, dins, unused) || itot.ins_sites != dins.recs.size() ||
            !merge_sites(seq, L.rc, L.slot_of_contig, L.cbase, P.sites, dins, o.min_alt, M))
            fail(HLMI_ESTATE, "%s: the sites' records do not fit the contigs", who);                                // (never)
        phase_ins_core(who, core, M, po, P.dev, reach, &keep);
        base->phase.ms_device = now_ms() - t_dev;
        if (!key_blocks(M, P.dev.blocks, P.dev.recs, o.min_side, kb)) fail(HLMI_ESTATE, "%s: a row's record names no block", who);     // (never)
        for (const KBlock &k : kb) any |= k.h.split;
        if (!any) polish_core(core, out);
        else {
            HapBlocksUp up;
            const size_t nb = P.dev.blocks.first.size();
            up.keys = true;
            up.gfirst.assign(nb, 0);
            up.glast.assign(nb, 0);
            up.split.assign(nb, 0);
            for (const KBlock &k : kb) {
                up.gfirst[k.h.block] = k.kf;
                up.glast[k.h.block] = k.kl;
                up.split[k.h.block] = k.h.split;
            }
            haplotig_core(who, core, L.cbase, keep, up, out);
        }
    }
    base->ms_device = now_ms() - t_dev;
    // the shared statistics, by hlmi_phase_ins's code: P.sites are the position sites, P.dev counts over the merged list
    phase_emit(who, R, P, po, {}, nullptr, nullptr, nullptr, &base->phase);
    st->slots_callable = itot.slots_callable;
    st->ins_sites = itot.ins_sites;
    st->ins_long = R.ins_long;
    st->ins_edge = R.ins_edge;
    st->ins_sites_phasing = M.ins_sites_phasing;
    st->ins_sites_left_out = M.ins_sites_left_out;
    st->ins_sites_phased = ins_sites_phased(M, P.dev.blocks);
    stat_set("variants_ins_slot_sites", (double)dins.slot_sites);

    std::vector<HapExtent> ext;
    ext.reserve(kb.size());
    for (const KBlock &k : kb) ext.push_back(HapExtent{k.h.contig, k.h.split, key_first_position(k.kf), key_last_position(k.kl), 0});
    const std::vector<std::string> lines = haplotig_records(who, R, o, any, out, ext, base);
    for (size_t i = 0; i < kb.size(); ++i) {
        kb[i].h.diff = ext[i].diff;
        if (!kb[i].h.split) continue;
        kb[i].diff_slots = diff_slots(out.open_pos, out.open_len, L.contigs.size(), kb[i].kf, kb[i].kl);
        st->diff_slots += kb[i].diff_slots;
    }
    write_lines(out_fa, lines);
    if (out_blocks) write_lines(out_blocks, haplotig_ins_block_lines(cs.names, kb));
}

}  // namespace

void haplotigs_ins_run(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts &o, int reach, const char *pairs_paf,
                       const char *out_fa, const char *out_blocks, hlmi_haplotig_ins_stats *st) {
    *st = hlmi_haplotig_ins_stats{};
    timed_call(&st->base, true, [&] {
        check_haplotig_opts("hlmi_haplotigs_ins", o);
        check_reach("hlmi_haplotigs_ins", reach);
        PileupRows R;
        rows_from_paf(contigs, reads, paf, plain_request("hlmi_haplotigs_ins", o.min_len, o.min_iden, pairs_paf), R);
        haplotigs_ins_body("hlmi_haplotigs_ins", R, o, reach, out_fa, out_blocks, st);
    });
    st->base.phase.ms_total = st->base.ms_total;
}

void haplotigs_reads_ins_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_haplotig_opts &o, int reach,
                             const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_ins_stats *st) {
    *st = hlmi_haplotig_ins_stats{};
    timed_call(&st->base, true, [&] {
        check_haplotig_opts("hlmi_haplotigs_reads_ins", o);
        check_reach("hlmi_haplotigs_reads_ins", reach);
        PileupRows R;
        rows_from_reads(contigs, reads, ao, plain_request("hlmi_haplotigs_reads_ins", o.min_len, o.min_iden, pairs_paf), R);
        haplotigs_ins_body("hlmi_haplotigs_reads_ins", R, o, reach, out_fa, out_blocks, st);
    });
    st->base.phase.ms_total = st->base.ms_total;
}

}  // namespace hlmi
