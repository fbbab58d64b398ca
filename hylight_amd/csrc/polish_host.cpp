// polish_host.cpp - two things (include/hylight_mi.h):
//   pol::rows_from_paf (polish_select.h), the PAF half of every pile-up call's row front: reading, the refusals, the row selection
//   (select_paf_rows), the layout (polish_layout: contigs side by side, tiles; rows_from_reads in polish_rows.hip calls it too),
//   the rows the device works on (sorted by contig and start) and their upload;
//   hlmi_polish and hlmi_polish_reads with their _q and _pairs forms: the option check, the request, one front each, and one
//   body - polish_core (polish.hip: the votes, the decisions and the bases), the statistics, the headers and the file.
// PARITY UNPINNED: racon is not part of the reference tree; tests/polish_model.py is the contract.
#include <algorithm>
#include <cstdio>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "paf_io.h"
#include "pair_list.h"
#include "polish_internal.h"
#include "polish_rows.h"
#include "polish_select.h"

namespace hlmi {

using namespace pol;

namespace {

// name -> first record of that name
std::unordered_map<std::string_view, uint32_t> first_records(const SeqSet &s, const char *path, const SelectNames &who) {
    std::unordered_map<std::string_view, uint32_t> m;
    m.reserve(s.size() * 2);
    for (size_t i = 0; i < s.size(); ++i) {
        if (s.len(i) >= MAX_SEQ) fail(HLMI_EINVAL, "%s: %s: %s has 2^28 bases or more", who.seqs, path, s.names[i].c_str());
        if (!m.emplace(s.names[i], (uint32_t)i).second && who.unique_names)
            fail(HLMI_EINVAL, "%s: %s: two records are named %s", who.seqs, path, s.names[i].c_str());
    }
    return m;
}

}  // namespace

namespace pol {

void select_paf_rows(const char *contigs, const char *reads, const char *paf, int min_len, double min_iden, const SelectNames &who,
                     PolQualCall *qc, PolPairCall *pc, PafSelection &out) {
    SeqSet &cs = out.cs, &rs = out.rs;
    PafText &pt = out.pt;
    std::vector<uint8_t> low;                                // hlmi_polish_q: per read record, its mean quality is below the floor
    read_seqs(contigs, cs);
    if (qc) low = polish_read_quals(who.quals, reads, qc->min_avg_qual, rs, out.rq, *qc);
    else read_seqs(reads, rs);
    const auto contig_named = first_records(cs, contigs, who), read_named = first_records(rs, reads, who);
    read_paf(paf, pt, false);
    const size_t n = pt.recs.size();
    // what read_paf lets through and this call does not: a row of 11 columns, a CIGAR that ends in a number
    std::vector<uint8_t> has_tag(n), is_star(n);
    for (size_t i = 0; i < n; ++i) {
        const std::string_view L = pt.line(i);
        if (std::count(L.begin(), L.end(), '\t') < 11) fail(HLMI_EINVAL, "%s:%zu: PAF row has 11 columns (< 12)", paf, i + 1);
        const std::string_view lf = L.substr(L.rfind('\t') + 1);
        has_tag[i] = lf.substr(0, 5) == "cg:Z:";
        is_star[i] = lf == "cg:Z:*";
        if (has_tag[i] && lf.back() >= '0' && lf.back() <= '9') fail(HLMI_EINVAL, "%s:%zu: cg:Z: ends in a number", paf, i + 1);
    }
    std::vector<int64_t> contig_of(pt.dict.names.size()), read_of(pt.dict.names.size());
    for (size_t k = 0; k < pt.dict.names.size(); ++k) {
        const auto c = contig_named.find(pt.dict.names[k]);
        const auto r = read_named.find(pt.dict.names[k]);
        contig_of[k] = c == contig_named.end() ? -1 : (int64_t)c->second;
        read_of[k] = r == read_named.end() ? -1 : (int64_t)r->second;
    }

    // hlmi_polish_pairs: the list (pair_list.h) over the names of this call.  What is wrong with the list itself is reported
    // behind the refusals of the rows below; until then no row is tested against it.
    std::string list_text;
    PairSet listed;
    std::unique_ptr<Error> list_error;
    std::vector<uint32_t> known_of;                          // PAF name id -> id among the call's names (every row's names are known)
    if (pc) {
        KnownNames known;
        known.add(rs.names);
        known.add(cs.names);
        try {
            list_text = read_file(pc->path);
            std::vector<PairLine> lines;
            if (const uint64_t bad = scan_pair_list(list_text, lines))
                fail(HLMI_EINVAL, "%s: %s:%llu: a list row has fewer than 6 fields", who.list, pc->path, (unsigned long long)bad);
            listed = make_pair_set(lines, known);
        } catch (const Error &e) {
            list_error = std::make_unique<Error>(e);
        }
        known_of.resize(pt.dict.names.size());
        for (size_t k = 0; k < pt.dict.names.size(); ++k) known_of[k] = (uint32_t)std::max<int64_t>(known.find(pt.dict.names[k]), 0);
        pc->pairs_listed = listed.listed;
        pc->pairs_unknown = listed.unknown;
        pc->rows_not_listed = 0;
    }

    // the refusals, row by row, and the selection
    std::unordered_map<uint32_t, PafSel> best;                  // query name -> its row so far
    for (size_t i = 0; i < n; ++i) {
        const PafRec &r = pt.recs[i];
        const uint32_t *op = pt.ops.data() + r.cig_off;
        if (!has_tag[i]) fail(HLMI_EINVAL, "%s:%zu: no cg:Z: tag in the last column", paf, i + 1);
        uint64_t n_t = 0, n_q = 0, n_eq = 0, n_all = 0;
        bool other = is_star[i] != 0;
        for (uint32_t k = 0; k < r.cig_n; ++k) {
            const uint64_t len = op[k] >> 4;
            const uint32_t code = op[k] & 15u;
            other |= code == OP_OTHER;
            n_all += len;
            if (code != OP_I) n_t += len;
            if (code != OP_D) n_q += len;
            if (code == OP_EQ) n_eq += len;
        }
        if (other) fail(HLMI_EINVAL, "%s:%zu: a CIGAR op other than = X I D", paf, i + 1);
        if (read_of[r.qid] < 0) fail(HLMI_EINVAL, "%s:%zu: query %s is not among the reads", paf, i + 1, pt.dict.names[r.qid].c_str());
        if (contig_of[r.tid] < 0) fail(HLMI_EINVAL, "%s:%zu: target %s is not among the contigs", paf, i + 1, pt.dict.names[r.tid].c_str());
        const uint32_t ci = (uint32_t)contig_of[r.tid], ri = (uint32_t)read_of[r.qid];
        if (r.qs > r.qe || r.qe > rs.len(ri) || r.ts > r.te || r.te > cs.len(ci))
            fail(HLMI_EINVAL, "%s:%zu: coordinates outside the sequences (read of %u, contig of %u bases)", paf, i + 1, rs.len(ri), cs.len(ci));
        if (n_t != (uint64_t)(r.te - r.ts)) fail(HLMI_EINVAL, "%s:%zu: the CIGAR has %llu target columns, te - ts = %u", paf, i + 1, (unsigned long long)n_t, r.te - r.ts);
        if (n_q != (uint64_t)(r.qe - r.qs)) fail(HLMI_EINVAL, "%s:%zu: the CIGAR has %llu query columns, qe - qs = %u", paf, i + 1, (unsigned long long)n_q, r.qe - r.qs);
        const uint32_t span = r.te - r.ts;
        if (r.qid == r.tid) continue;
        if (!low.empty() && low[ri]) { ++qc->rows_low_qual; continue; }
        if (pc && !list_error && !listed.has(known_of[r.qid], known_of[r.tid])) { ++pc->rows_not_listed; continue; }
        if (span == 0 || (int64_t)span < (int64_t)min_len) continue;
        if ((double)n_eq / (double)n_all < min_iden) continue;
        const auto it = best.find(r.qid);
        if (it == best.end()) best.emplace(r.qid, PafSel{i, ci, ri});
        else if (span > pt.recs[it->second.line].te - pt.recs[it->second.line].ts) it->second = PafSel{i, ci, ri};
    }
    if (list_error) throw *list_error;
    std::vector<PafSel> &sel = out.sel;
    sel.clear();
    sel.reserve(best.size());
    for (const auto &kv : best) sel.push_back(kv.second);
    std::sort(sel.begin(), sel.end(), [&](const PafSel &a, const PafSel &b) {      // by (contig, start), the line last
        if (a.contig != b.contig) return a.contig < b.contig;
        const uint32_t sa = pt.recs[a.line].ts, sb = pt.recs[b.line].ts;
        return sa != sb ? sa < sb : a.line < b.line;
    });
}

// in.rows, in.ops, in.reads and, when weighted, in.quals from the selection, in its order; L is polish_layout's over the same
// rows.  Adds the rows' ins_edge and ins_long to the two counters.
static void paf_rows_input(const PafSelection &S, const PolLayout &L, bool weighted, PolDevIn &in, uint64_t &ins_edge, uint64_t &ins_long) {
    const PafText &pt = S.pt;
    const SeqSet &rs = S.rs;
    in.rows.reserve(S.sel.size());
    for (const PafSel &s : S.sel) {
        const PafRec &r = pt.recs[s.line];
        const uint32_t *op = pt.ops.data() + r.cig_off;
        PolRow row{};
        row.read_off = in.reads.size();
        row.cig_off = in.ops.size();
        row.ts = r.ts; row.te = r.te; row.qn = r.qe - r.qs;
        row.rev = (r.flags & PF_REV) ? 1u : 0u;
        row.cbase = L.cbase[L.slot_of_contig[s.contig]];
        in.reads.append(rs.bases, rs.off[s.read] + r.qs, row.qn);
        if (weighted) in.quals.append(S.rq.quals, rs.off[s.read] + r.qs, row.qn);
        RowWalk w;                                           // polish_rows.h: drop, merge, ins_edge, ins_long
        RowOp done;
        row_walk_begin(w, r.ts, r.te);
        for (uint32_t k = 0; k < r.cig_n; ++k)
            if (row_walk_op(w, op[k], &done)) in.ops.push_back(done.word);
        if (row_walk_end(w, &done)) in.ops.push_back(done.word);
        ins_edge += w.ins_edge;
        ins_long += w.ins_long;
        row.cig_n = w.n_out;
        in.rows.push_back(row);
    }
}

void rows_from_paf(const char *contigs, const char *reads, const char *paf, const RowsRequest &q, PileupRows &R) {
    PafSelection &S = R.paf;
    PolQualCall checked;                        // check_quals: no floor and no weights, the quality strings are only checked
    R.pc.path = q.pairs_paf;
    select_paf_rows(contigs, reads, paf, q.min_len, q.min_iden, q.who, q.qc ? q.qc : q.check_quals ? &checked : nullptr,
                    q.pairs_paf ? &R.pc : nullptr, S);
    R.n_rows = S.pt.recs.size();
    R.n_sel = S.sel.size();
    polish_check_weight_width(q.who.quals, q.qc, R.n_sel);

    // the device's input: polished contigs side by side, the aligned stretch of every read, compact CIGARs, tiles
    std::vector<PolSpan> spans;
    spans.reserve(S.sel.size());
    for (const PafSel &s : S.sel) spans.push_back(PolSpan{s.contig, S.pt.recs[s.line].ts, S.pt.recs[s.line].te});
    PolLayout &L = R.L;
    polish_layout(S.cs, spans, q.who.seqs, L, !q.spans_only);
    if (q.spans_only) {
        R.t_dev = now_ms();
        if (spans.empty()) return;
        R.d_spans.upload(spans);
        return R.upload_tiles();
    }
    PolDevIn in;
    refill_missing_quals(q, S.rs, S.rq);
    paf_rows_input(S, L, quals_travel(q), in, R.ins_edge, R.ins_long);
    in.contigs = std::move(L.contigs);
    in.cbase = L.cbase;
    in.tiles = std::move(L.tiles);
    R.t_dev = now_ms();
    polish_upload(in, R.up);
    L.contigs = std::move(in.contigs);
}

}  // namespace pol

namespace {

// what both entry points do behind the rows: the votes, the decisions and the bases (polish.hip), the statistics, the headers
// and the file
void polish_body(PileupRows &R, const hlmi_polish_opts &o, const char *out_fa, hlmi_polish_stats *st) {
    const SeqSet &cs = R.cs();
    const PolLayout &L = R.L;
    set_row_stats(R, st);
    st->contigs_polished = L.cbase.size() - 1;
    st->ins_edge = R.ins_edge;
    st->ins_long = R.ins_long;
    R.up.core.min_cov = o.min_cov;
    PolDevOut out;
    polish_core(R.up.core, out);
    st->ms_device = now_ms() - R.t_dev;

    std::vector<std::string> lines;
    for (uint32_t c = 0; c < cs.size(); ++c) {
        if (!L.rc[c]) {
            if (o.include_unpolished && cs.len(c)) {
                lines.push_back(">" + cs.names[c]);
                lines.push_back(cs.bases.substr(cs.off[c], cs.len(c)));
            }
            continue;
        }
        const uint32_t j = L.slot_of_contig[c], b = L.cbase[j], len = cs.len(c);
        const uint64_t covered = count_decisions(out, b, L.contigs.data() + b, len, st);
        const uint64_t new_len = out.start[j + 1] - out.start[j];
        if (!new_len) continue;
        char head[96];
        snprintf(head, sizeof head, " LN:i:%llu RC:i:%u XC:f:%.6f", (unsigned long long)new_len, L.rc[c], (double)covered / (double)len);
        lines.push_back(">" + cs.names[c] + head);
        lines.push_back(out.bases.substr(out.start[j], new_len));
    }
    write_lines(out_fa, lines);
}

}  // namespace

void polish_run(const char *contigs, const char *reads, const char *paf, const hlmi_polish_opts &o, const char *out_fa,
                hlmi_polish_stats *st, PolQualCall *qc, PolPairCall *pc) {
    timed_call(st, false, [&] {                 // false: hlmi_polish, _q and _pairs alone leave hlmi_last_stats_json's stats as they are
        if (o.min_cov < 1) fail(HLMI_EINVAL, "hlmi_polish: min_cov %d (< 1)", o.min_cov);
        PileupRows R;
        rows_from_paf(contigs, reads, paf, RowsRequest{SelectNames{}, o.min_len, o.min_iden, qc, pc ? pc->path : nullptr}, R);
        if (pc) *pc = R.pc;
        polish_body(R, o, out_fa, st);
    });
}

void polish_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_polish_opts &o, const char *out_fa,
                      hlmi_polish_stats *st, PolQualCall *qc, PolPairCall *pc) {
    timed_call(st, true, [&] {
        if (o.min_cov < 1) fail(HLMI_EINVAL, "hlmi_polish_reads: min_cov %d (< 1)", o.min_cov);
        PileupRows R;
        rows_from_reads(contigs, reads, ao,
                        RowsRequest{SelectNames{"hlmi_polish_reads", "hlmi_polish_reads_q", "hlmi_polish_reads_pairs", true}, o.min_len,
                                    o.min_iden, qc, pc ? pc->path : nullptr}, R);
        if (pc) *pc = R.pc;
        polish_body(R, o, out_fa, st);
    });
}

namespace pol {

std::vector<uint8_t> polish_read_quals(const char *who, const char *reads, double min_avg_qual, SeqSet &rs, SeqQual &rq, PolQualCall &qc) {
    if (!(min_avg_qual >= 0.0)) fail(HLMI_EINVAL, "%s: min_avg_qual %g (negative or not a number)", who, min_avg_qual);
    read_seqs_qual(reads, rs, rq);
    QualFacts f = quality_facts(rs, rq, min_avg_qual);
    if (f.bad_kind == 1)
        fail(HLMI_EINVAL, "%s: %s: record %s has %u bases and %llu quality bytes", who, reads, rs.names[f.bad_rec].c_str(),
             rs.len(f.bad_rec), (unsigned long long)rq.qual_len[f.bad_rec]);
    if (f.bad_kind == 2)
        fail(HLMI_EINVAL, "%s: %s: record %s: quality byte %u at base %llu (outside 33..126)", who, reads, rs.names[f.bad_rec].c_str(),
             (unsigned)f.bad_byte, (unsigned long long)f.bad_at);
    qc.reads_with_qual = f.reads_with_qual;
    qc.rows_low_qual = 0;
    return std::move(f.low);
}

void polish_check_weight_width(const char *who, const PolQualCall *qc, uint64_t rows_selected) {
    if (qc && qc->qual_weight && !weight_sums_fit(rows_selected))
        fail(HLMI_EINVAL, "%s: %llu selected rows of weight 93 at the most do not fit the 32-bit sums", who, (unsigned long long)rows_selected);
}

void polish_layout(const SeqSet &cs, const std::vector<PolSpan> &sel, const char *who, PolLayout &L, bool with_bytes) {
    L = PolLayout{};
    L.rc.assign(cs.size(), 0);
    L.slot_of_contig.assign(cs.size(), 0);
    for (const PolSpan &s : sel) ++L.rc[s.contig];
    uint32_t n_polished = 0;
    uint64_t total = 0;
    for (uint32_t c = 0; c < cs.size(); ++c)
        if (L.rc[c]) {
            L.slot_of_contig[c] = n_polished++;
            if (total + cs.len(c) >= (1ull << 31)) fail(HLMI_EINVAL, "%s: 2^31 contig bases or more to polish in one call", who);
            L.cbase.push_back((uint32_t)total);
            if (with_bytes) L.contigs.append(cs.bases, cs.off[c], cs.len(c));
            total += cs.len(c);
        }
    L.cbase.push_back((uint32_t)total);
    for (size_t r0 = 0; r0 < sel.size();) {
        size_t r1 = r0;
        while (r1 < sel.size() && sel[r1].contig == sel[r0].contig) ++r1;
        const uint32_t cbase = L.cbase[L.slot_of_contig[sel[r0].contig]], len = cs.len(sel[r0].contig);
        size_t lo = r0, hi = r0;
        for (uint32_t t0 = 0; t0 < len; t0 += POLISH_TILE) {
            const uint32_t n_pos = std::min<uint32_t>(POLISH_TILE, len - t0);
            while (hi < r1 && sel[hi].ts < t0 + n_pos) ++hi;
            while (lo < hi && sel[lo].te <= t0) ++lo;            // (rows behind lo that ended too are passed over by the kernel)
            if (lo < hi) L.tiles.push_back(PolTile{t0, n_pos, (uint32_t)lo, (uint32_t)hi, cbase});
        }
        r0 = r1;
    }
}

}  // namespace pol

}  // namespace hlmi
