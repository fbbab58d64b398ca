// haplotigs_host.cpp - the host part of hlmi_haplotigs and hlmi_haplotigs_reads (include/hylight_mi.h): the contigs polished once
// per side of every split block.  The rows come from the pile-up calls' row front (polish_select.h), sites and phasing are
// hlmi_phase's (phase_device, phase_emit for the statistics), called and not restated; the split rule, the blocks file and
// the headers are haplotigs_text.h's, the exclusion intervals and the two-sided passes haplotigs.hip's.  With no split block the
// single-sided polish_core gives the bytes and no kernel of haplotigs.hip runs.  The _reach calls hand `reach` down to the
// phasing and are the same body otherwise: blocks stay runs of consecutive sites, a row's side comes from its record.
// haplotig_records - the records of out_fa and the statistics they carry - and the option refusals are shared with the _ins
// calls (haplotigs_ins_host.cpp), whose phasing in front is hlmi_phase_ins's.
// PARITY UNPINNED: a function of the project's own; tests/haplotigs_model.py is the contract.
#include <algorithm>
#include <string>
#include <vector>

#include "ava.h"
#include "common.h"
#include "haplotigs_internal.h"
#include "paf_io.h"
#include "phase_internal.h"
#include "polish_internal.h"
#include "polish_select.h"

namespace hlmi {

using namespace pol;
using namespace ph;
using namespace hap;

namespace hap {

hlmi_phase_opts phase_part(const hlmi_haplotig_opts &o) {
    return hlmi_phase_opts{o.min_len, o.min_iden, o.min_cov, o.min_alt, o.min_frac, o.min_link, o.min_agree};
}

void check_haplotig_opts(const char *who, const hlmi_haplotig_opts &o) {
    check_phase_opts(who, phase_part(o));
    if (o.min_side < 1) fail(HLMI_EINVAL, "%s: min_side %d (< 1)", who, o.min_side);
}

std::vector<std::string> haplotig_records(const char *who, const PileupRows &R, const hlmi_haplotig_opts &o, bool any, const PolDevOut &out,
                                          std::vector<HapExtent> &ext, hlmi_haplotig_stats *st) {
    const SeqSet &cs = R.cs();
    const PolLayout &L = R.L;
    const size_t G = L.contigs.size(), n = L.cbase.size() - 1;
    if (out.start.size() != (any ? 2 * n : n) + 1 || out.sym.size() != (any ? 2 * G : G) || out.open_len.size() != out.open_pos.size())
        fail(HLMI_ESTATE, "%s: the consensus does not fit the contigs", who);                                        // (never)
    std::vector<std::string> lines;
    size_t k = 0;                               // ext's blocks of the contigs so far
    for (uint32_t c = 0; c < cs.size(); ++c) {
        if (!L.rc[c]) {
            if (o.include_unpolished && cs.len(c)) {
                lines.push_back(">" + cs.names[c]);
                lines.push_back(cs.bases.substr(cs.off[c], cs.len(c)));
                ++st->records;
            }
            continue;
        }
        const uint32_t j = L.slot_of_contig[c], b = L.cbase[j], len = cs.len(c);
        const size_t k0 = k;
        uint64_t n_split = 0, inside = 0;
        for (; k < ext.size() && ext[k].contig == c; ++k)
            if (ext[k].split) {
                ++n_split;
                inside += (uint64_t)ext[k].glast - ext[k].gfirst + 1;
            }
        for (size_t side = 0; side < (n_split ? 2u : 1u); ++side) {
            const size_t g0 = side * G + b;
            const uint64_t covered = count_decisions(out, g0, L.contigs.data() + b, len, st);
            const uint64_t at = out.start[side * n + j], new_len = out.start[side * n + j + 1] - at;
            if (!new_len) continue;
            lines.push_back(haplotig_head(cs.names[c], n_split ? "AB"[side] : '\0', new_len, L.rc[c], covered, len, n_split, inside));
            lines.push_back(out.bases.substr(at, new_len));
            ++st->records;
        }
        if (!n_split) continue;
        ++st->contigs_split;
        st->blocks_split += n_split;
        st->positions_split += inside;
        for (size_t i = k0; i < k; ++i)
            if (ext[i].split) {
                ext[i].diff = diff_positions(out.sym, G, ext[i].gfirst, ext[i].glast);
                st->diff_positions += ext[i].diff;
            }
    }
    return lines;
}

}  // namespace hap

namespace {

// What the entry points do behind the rows: the phasing, the split rule, one or two sides of consensus, the statistics and the
// two files.  reach 0: the plain calls
void haplotigs_body(const char *who, PileupRows &R, const hlmi_haplotig_opts &o, const char *out_fa, const char *out_blocks,
                    hlmi_haplotig_stats *st, int reach = 0) {
    const SeqSet &cs = R.cs();
    const PolLayout &L = R.L;
    const double t_dev = R.t_dev;
    const hlmi_phase_opts po = phase_part(o);
    set_row_stats(R, &st->phase);
    st->ins_edge = R.ins_edge;
    st->ins_long = R.ins_long;
    PolCoreIn &core = R.up.core;
    core.min_cov = o.min_cov;
    core.quals = nullptr;
    Phased P;
    std::vector<HBlock> hb;
    PolDevOut out;
    bool any = false;
    {
        DevRecs keep;
        phase_device(who, R, po, P, &keep, reach);
        st->phase.ms_device = now_ms() - t_dev;
        if (!haplotig_blocks(P.sites, P.dev.blocks, P.dev.recs, o.min_side, hb)) fail(HLMI_ESTATE, "%s: a row's record names no block", who);   // (never)
        for (const HBlock &h : hb) any |= h.split;
        if (!any) polish_core(core, out);
        else {
            HapBlocksUp up;
            const size_t nb = P.dev.blocks.first.size();
            up.gfirst.assign(nb, 0);
            up.glast.assign(nb, 0);
            up.split.assign(nb, 0);
            for (const HBlock &h : hb) {
                up.gfirst[h.block] = h.gfirst;
                up.glast[h.block] = h.glast;
                up.split[h.block] = h.split;
            }
            haplotig_core(who, core, L.cbase, keep, up, out);
        }
    }
    st->ms_device = now_ms() - t_dev;
    phase_emit(who, R, P, po, {}, nullptr, nullptr, nullptr, &st->phase);

    std::vector<HapExtent> ext;
    ext.reserve(hb.size());
    for (const HBlock &h : hb) ext.push_back(HapExtent{h.contig, h.split, h.gfirst, h.glast, 0});
    const std::vector<std::string> lines = haplotig_records(who, R, o, any, out, ext, st);
    for (size_t i = 0; i < hb.size(); ++i) hb[i].diff = ext[i].diff;
    write_lines(out_fa, lines);
    if (out_blocks) write_lines(out_blocks, haplotig_block_lines(cs.names, hb));
}

}  // namespace

void haplotigs_run(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts &o, const char *pairs_paf,
                   const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st) {
    timed_call(st, true, [&] {
        check_haplotig_opts("hlmi_haplotigs", o);
        PileupRows R;
        rows_from_paf(contigs, reads, paf, plain_request("hlmi_haplotigs", o.min_len, o.min_iden, pairs_paf), R);
        haplotigs_body("hlmi_haplotigs", R, o, out_fa, out_blocks, st);
    });
    st->phase.ms_total = st->ms_total;
}

void haplotigs_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_haplotig_opts &o, const char *pairs_paf,
                         const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st) {
    timed_call(st, true, [&] {
        check_haplotig_opts("hlmi_haplotigs_reads", o);
        PileupRows R;
        rows_from_reads(contigs, reads, ao, plain_request("hlmi_haplotigs_reads", o.min_len, o.min_iden, pairs_paf), R);
        haplotigs_body("hlmi_haplotigs_reads", R, o, out_fa, out_blocks, st);
    });
    st->phase.ms_total = st->ms_total;
}

void haplotigs_reach_run(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts &o, int reach, const char *pairs_paf,
                         const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st) {
    timed_call(st, true, [&] {
        check_haplotig_opts("hlmi_haplotigs_reach", o);
        check_reach("hlmi_haplotigs_reach", reach);
        PileupRows R;
        rows_from_paf(contigs, reads, paf, plain_request("hlmi_haplotigs_reach", o.min_len, o.min_iden, pairs_paf), R);
        haplotigs_body("hlmi_haplotigs_reach", R, o, out_fa, out_blocks, st, reach);
    });
    st->phase.ms_total = st->ms_total;
}

void haplotigs_reads_reach_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_haplotig_opts &o, int reach,
                               const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st) {
    timed_call(st, true, [&] {
        check_haplotig_opts("hlmi_haplotigs_reads_reach", o);
        check_reach("hlmi_haplotigs_reads_reach", reach);
        PileupRows R;
        rows_from_reads(contigs, reads, ao, plain_request("hlmi_haplotigs_reads_reach", o.min_len, o.min_iden, pairs_paf), R);
        haplotigs_body("hlmi_haplotigs_reads_reach", R, o, out_fa, out_blocks, st, reach);
    });
    st->phase.ms_total = st->ms_total;
}

}  // namespace hlmi
