// polish_rows.hip - hlmi_polish_reads (include/hylight_mi.h): hlmi_ava and hlmi_polish in one call, without the PAF between
// them.  The overlapper's rows stay in HBM (ava_device: AvaRows, in the order of the lines hlmi_ava writes - a row's index IS its
// PAF line), and what polish_host.cpp does with the parsed text happens where the rows are:
//   pr_facts_kernel    a wave per row: n_eq and n_all over the row's ops, the selection rules in polish_host.cpp's order, and a
//                      surviving row claims its read with one 64-bit atomicMax on span << 32 | ~row (largest span, earliest line)
//   pr_winner_kernel   a thread per row: is it the one its read kept?  (flag-select: the winners, ascending by line)
//   pr_key_kernel      a thread per winner: contig record << 28 | ts; a stable radix sort gives the order (contig, ts, line)
//   pr_count_kernel    a thread per winner walks its CIGAR with the rule of polish_rows.h: ops of the compact CIGAR, ins_edge,
//                      ins_long, and the (contig, ts, te) the host lays the tiles out from - all that comes back of the rows
//   pr_write_kernel    the same walk once more behind a scan: the compact ops and the PolRow table
// The reads are voted from the overlapper's resident codes (PolRow::read_off points into DevReads::codes()); the votes, the
// decisions and the bases are polish.hip's (polish_core), layout, headers and file polish_host.cpp's (polish_layout, polish_body).
// hlmi_polish_reads_q: the resident reads hold codes only, so the quality bytes go up as one array at the offsets of
// DevReads::codes() (PolRow::read_off indexes both), and the read floor is one byte per name rank that pr_facts_kernel looks up.
// hlmi_polish_reads_pairs: the list becomes a sorted array of keys qid << 32 | tid on the device (polish_pairs.hip), and
// pr_facts_kernel looks a row's key up with the whole wave (wave_search.h) directly behind the floor.
//
// All of it is pol::rows_from_reads (polish_select.h), the aligned half of the row front of every pile-up call: the first three
// kernels with the flag-select and the sort are select_device_rows, the last two with the layout's uploads device_rows_input.
// hlmi_depth_reads asks for spans only: depth.hip's depth_spans_from_rows then stands in for the two CIGAR kernels.  No entry
// point lives here: every _reads call is in its family's host file.
//
// Why a wave per row in the first kernel and a thread per row in the last two: the first reads the ops of EVERY row (all of
// the CIGAR traffic of this file), needs two sums and nothing else of them, so 64 consecutive words per load and a DPP sum fit;
// the walk of polish_rows.h is sequential by nature (an op's fate depends on the op before it), runs over the winners only (one
// row per read at most) and shares its code with the host - a thread reads its row's words one behind the other, 16 to a
// cache line.  Every loop is bounded by a count known at its head.
#include <hip/hip_runtime.h>

#include "ava.h"
#include "common.h"
#include "depth_internal.h"
#include "dev_prims.h"
#include "paf_io.h"
#include "phase_internal.h"
#include "polish_internal.h"
#include "polish_rows.h"
#include "polish_select.h"
#include "wave_ops.h"
#include "wave_search.h"

namespace hlmi {

using namespace pol;

namespace {

static_assert(ROW_OP_I == OP_I && ROW_INS_CAP == (uint32_t)POLISH_INS_CAP, "polish_rows.h restates two constants");

constexpr int WG = 256, WAVES = WG / 64;
constexpr unsigned MAX_GRID = 1u << 16;         // blocks of a strided launch
constexpr uint32_t NO_REC = 0xffffffffu;
inline dim3 grid1(size_t n) { return dim3((unsigned)std::min<size_t>(cdiv(n ? n : 1, WG), MAX_GRID)); }

__global__ __launch_bounds__(WG) void pr_facts_kernel(const PafRec *__restrict__ recs, size_t n_rows, const uint32_t *__restrict__ ops_base,
                                                      int min_len, double min_iden, unsigned long long *__restrict__ best,
                                                      const uint8_t *__restrict__ low_of_rank, unsigned long long *__restrict__ n_low,
                                                      const uint64_t *__restrict__ pair_keys, size_t n_keys,
                                                      unsigned long long *__restrict__ n_unlisted) {
    const int lane = threadIdx.x & 63;
    const size_t n_waves = (size_t)gridDim.x * WAVES;
    for (size_t i = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); i < n_rows; i += n_waves) {
        const PafRec r = recs[i];
        const uint32_t span = r.te - r.ts;
        if (r.qid == r.tid) continue;                                                           // (the same in every lane)
        if (low_of_rank && low_of_rank[r.qid]) {        // the read floor (nullptr: off): the row claims nothing, and is counted
            if (lane == 0) atomicAdd(n_low, 1ull);
            continue;
        }
        if (pair_keys && !wave_contains_u64(pair_keys, n_keys, (uint64_t)r.qid << 32 | r.tid)) {    // the pair list (nullptr: off)
            if (lane == 0) atomicAdd(n_unlisted, 1ull);
            continue;
        }
        if (span == 0 || (int64_t)span < (int64_t)min_len) continue;
        const uint32_t *o = ops_base + r.cig_off;
        uint32_t eq = 0, all = 0;               // a row's op lengths add up to less than 2^29 (two sequences below 2^28)
        for (uint32_t k0 = 0; k0 < r.cig_n; k0 += 64) {
            const uint32_t k = k0 + (uint32_t)lane;
            const uint32_t w = k < r.cig_n ? o[k] : 0u;
            all += w >> 4;
            eq += (w & 15u) == OP_EQ ? w >> 4 : 0u;
        }
        const uint32_t n_eq = (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum_incl_dpp(eq), 63);
        const uint32_t n_all = (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum_incl_dpp(all), 63);
        if ((double)n_eq / (double)n_all < min_iden) continue;                                  // one IEEE division, as on the host
        if (lane == 0) atomicMax(&best[r.qid], (unsigned long long)span << 32 | (uint32_t)~(uint32_t)i);
    }
}

// A row that did not survive never claimed; a read nobody claimed holds 0, whose low word no row's ~index equals (fewer than
// 2^32 rows).
__global__ __launch_bounds__(WG) void pr_winner_kernel(const PafRec *__restrict__ recs, size_t n_rows,
                                                       const unsigned long long *__restrict__ best, uint8_t *__restrict__ flag) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n_rows; i += step)
        flag[i] = (uint32_t)best[recs[i].qid] == (uint32_t)~(uint32_t)i;
}

__global__ __launch_bounds__(WG) void pr_key_kernel(const PafRec *__restrict__ recs, const uint32_t *__restrict__ idx, size_t n_sel,
                                                    const uint32_t *__restrict__ crec_of_rank, uint64_t *__restrict__ key) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < n_sel; j += step) {
        const PafRec r = recs[idx[j]];
        key[j] = (uint64_t)crec_of_rank[r.tid] << 28 | r.ts;                    // ts < 2^28
    }
}

// totals[0] += ins_edge, totals[1] += ins_long
__global__ __launch_bounds__(WG) void pr_count_kernel(const PafRec *__restrict__ recs, const uint32_t *__restrict__ idx, size_t n_sel,
                                                      const uint32_t *__restrict__ ops_base, const uint32_t *__restrict__ crec_of_rank,
                                                      uint32_t *__restrict__ cig_n, PolSpan *__restrict__ span,
                                                      unsigned long long *__restrict__ totals) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < n_sel; j += step) {
        const PafRec r = recs[idx[j]];
        const uint32_t *o = ops_base + r.cig_off;
        RowWalk w;
        RowOp done;
        row_walk_begin(w, r.ts, r.te);
        for (uint32_t k = 0; k < r.cig_n; ++k) row_walk_op(w, o[k], &done);
        row_walk_end(w, &done);
        cig_n[j] = w.n_out;
        span[j] = PolSpan{crec_of_rank[r.tid], r.ts, r.te};
        if (w.ins_edge) atomicAdd(&totals[0], (unsigned long long)w.ins_edge);
        if (w.ins_long) atomicAdd(&totals[1], (unsigned long long)w.ins_long);
    }
}

__global__ __launch_bounds__(WG) void pr_write_kernel(const PafRec *__restrict__ recs, const uint32_t *__restrict__ idx, size_t n_sel,
                                                      const uint32_t *__restrict__ ops_base, const uint32_t *__restrict__ crec_of_rank,
                                                      const uint32_t *__restrict__ qrec_of_rank, const uint64_t *__restrict__ q_off,
                                                      const uint32_t *__restrict__ cbase_of_crec, uint32_t n_crec,
                                                      const uint64_t *__restrict__ cig_off, const uint32_t *__restrict__ cig_n,
                                                      PolRow *__restrict__ rows, uint32_t *__restrict__ ops_out) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < n_sel; j += step) {
        const PafRec r = recs[idx[j]];
        const uint32_t *o = ops_base + r.cig_off;
        const uint64_t off = cig_off[j];
        const uint32_t n = cig_n[j];            // what the count pass found: no op is written behind it
        RowWalk w;
        RowOp done;
        row_walk_begin(w, r.ts, r.te);
        for (uint32_t k = 0; k < r.cig_n; ++k)
            if (row_walk_op(w, o[k], &done) && w.n_out <= n) ops_out[off + w.n_out - 1] = done.word;
        if (row_walk_end(w, &done) && w.n_out <= n) ops_out[off + w.n_out - 1] = done.word;
        const uint32_t crec = crec_of_rank[r.tid];
        PolRow row;
        row.read_off = q_off[qrec_of_rank[r.qid]] + r.qs;
        row.cig_off = off;
        row.cig_n = n;
        row.ts = r.ts; row.te = r.te; row.qn = r.qe - r.qs;
        row.rev = (r.flags & PF_REV) ? 1u : 0u;
        row.cbase = crec < n_crec ? cbase_of_crec[crec] : 0u;
        rows[j] = row;
    }
}

// the bases the encoder folded into T for the aligner and the ASCII vote does not count (U, u): code 4 from here on
__global__ __launch_bounds__(WG) void pr_unvote_kernel(uint8_t *__restrict__ codes, const uint64_t *__restrict__ at, size_t n) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += step) codes[at[i]] = 4;
}

// the refusals that need the sequences only: 2^28 bases, a name twice in one file; -> name rank -> record (NO_REC: none)
std::vector<uint32_t> record_of_rank(const SeqSet &s, const std::vector<uint32_t> &rank, size_t n_ranks, const char *path, const char *who) {
    std::vector<uint32_t> rec(n_ranks, NO_REC);
    for (size_t i = 0; i < s.size(); ++i) {
        if (s.len(i) >= MAX_SEQ) fail(HLMI_EINVAL, "%s: %s: %s has 2^28 bases or more", who, path, s.names[i].c_str());
        if (rec[rank[i]] != NO_REC) fail(HLMI_EINVAL, "%s: %s: two records are named %s", who, path, s.names[i].c_str());
        rec[rank[i]] = (uint32_t)i;
    }
    return rec;
}

}  // namespace

namespace pol {

void select_device_rows(const char *contigs, const char *reads, const hlmi_ava_opts &ao, int min_len, double min_iden,
                        const SelectNames &who, PolQualCall *qc, PolPairCall *pc, RowSelection &out) {
    if (ao.stub_oh >= 0) fail(HLMI_EINVAL, "%s: stub_oh %d: the bare rows of stub candidates have no CIGAR", who.seqs, ao.stub_oh);
    SeqSet &cs = out.cs, &rs = out.rs;
    std::vector<uint8_t> low;                   // hlmi_polish_reads_q: per read record, its mean quality is below the floor
    read_seqs(contigs, cs);
    if (qc) low = polish_read_quals(who.quals, reads, qc->min_avg_qual, rs, out.rq, *qc);
    else read_seqs(reads, rs);
    out.t_dev = now_ms();
    AvaPairCall &call = out.call;
    call.setup(cs, rs, ao);
    const size_t n_ranks = call.name_of_rank.size();
    out.crec_of_rank = record_of_rank(cs, call.rt, n_ranks, contigs, who.seqs);      // (refusals: before the overlapper runs)
    out.qrec_of_rank = record_of_rank(rs, call.rq, n_ranks, reads, who.seqs);
    AvaRows &rows = out.rows;
    ava_device(call.in, ao, rows);
    const size_t R = rows.n_rows;
    if (R >= (1ull << 32)) fail(HLMI_EINVAL, "%s: %zu overlapper rows (2^32 and more)", who.seqs, R);
    out.n_rows = R;
    PairKeys pk;                                // hlmi_polish_reads_pairs: the list's own refusal comes behind the ones above
    if (pc) pair_keys_device(who.list, call.name_of_rank, *pc, pk);

    size_t S = 0;
    DBuf<uint32_t> &idx = out.idx;
    idx.alloc(std::max<size_t>(R, 1));
    if (R) {
        KTimer kt("polish_rows");
        DBuf<unsigned long long> best(n_ranks);
        DBuf<uint8_t> flag(R), d_low;
        DBuf<unsigned long long> n_low(2);      // rows of low reads, rows whose pair is not listed
        best.zero();
        n_low.zero();
        if (!low.empty()) {
            std::vector<uint8_t> low_of_rank(n_ranks, 0);
            for (size_t i = 0; i < rs.size(); ++i) low_of_rank[call.rq[i]] = low[i];
            d_low.upload(low_of_rank);
        }
        // a wave per row up to MAX_GRID workgroups (262 144 rows), then a wave takes several; the hook lowers the cap so that
        // the tests reach that with a few dozen rows
        unsigned facts_grid = MAX_GRID;
        if (const char *e = hook("HLMI_POLISH_ROWS_GRID")) facts_grid = (unsigned)std::min<long>(std::max<long>(1, atol(e)), MAX_GRID);
        hipLaunchKernelGGL(pr_facts_kernel, dim3((unsigned)std::min<size_t>(cdiv(R, WAVES), facts_grid)), dim3(WG), 0, stream(), rows.recs.p,
                           R, rows.ops_base, min_len, min_iden, best.p, low.empty() ? nullptr : d_low.p, n_low.p,
                           pc ? pk.keys.p : nullptr, pk.n, n_low.p + 1);
        hipLaunchKernelGGL(pr_winner_kernel, grid1(R), dim3(WG), 0, stream(), rows.recs.p, R, best.p, flag.p);
        HIP_CHECK(hipGetLastError());
        S = select_flagged_indices(flag.p, idx.p, R);
        if (qc) qc->rows_low_qual = download_one(n_low.p);
        if (pc) pc->rows_not_listed = download_one(n_low.p + 1);
    }
    out.n_sel = S;
    if (S) {                                    // the order (contig, ts, line): the select left the lines ascending, the sort is stable
        KTimer kt("polish_rows");
        out.d_crec_of_rank.upload(out.crec_of_rank);
        out.d_qrec_of_rank.upload(out.qrec_of_rank);
        DBuf<uint64_t> key(S);
        hipLaunchKernelGGL(pr_key_kernel, grid1(S), dim3(WG), 0, stream(), rows.recs.p, idx.p, S, out.d_crec_of_rank.p, key.p);
        HIP_CHECK(hipGetLastError());
        sort_pairs_u64_u32(key.p, idx.p, S, 0, 28 + bits_for(cs.size() - 1));
    }
}

// The selected rows as PolRow, compact CIGARs and the layout, where the rows are.  R.dev is selected; weighted: the quality
// bytes go up beside the overlapper's codes.
static void device_rows_input(PileupRows &R, const char *who, bool weighted) {
    const RowSelection &sel = R.dev;
    const SeqSet &cs = sel.cs, &rs = sel.rs;
    const SeqQual &rq = sel.rq;
    const AvaPairCall &call = sel.call;
    const AvaRows &rows = sel.rows;
    const DBuf<uint32_t> &idx = sel.idx, &d_crec_of_rank = sel.d_crec_of_rank, &d_qrec_of_rank = sel.d_qrec_of_rank;
    const size_t S = sel.n_sel;
    PolLayout &L = R.L;
    PolUploaded &out = R.up;

    // ---- the compact CIGARs' sizes and the spans --------------------------------------------------------------------------------
    std::vector<PolSpan> spans;
    DBuf<uint32_t> cig_n(std::max<size_t>(S, 1));
    DBuf<uint64_t> cig_off(std::max<size_t>(S, 1));
    uint64_t n_ops = 0;
    if (S) {
        KTimer kt("polish_rows");
        DBuf<PolSpan> d_span(S);
        DBuf<unsigned long long> totals(2);
        totals.zero();
        hipLaunchKernelGGL(pr_count_kernel, grid1(S), dim3(WG), 0, stream(), rows.recs.p, idx.p, S, rows.ops_base, d_crec_of_rank.p,
                           cig_n.p, d_span.p, totals.p);
        HIP_CHECK(hipGetLastError());
        exclusive_scan_u32_to_u64(cig_n.p, cig_off.p, S);
        n_ops = download_one(cig_off.p + (S - 1)) + download_one(cig_n.p + (S - 1));
        const std::vector<unsigned long long> t = totals.download(2);
        R.ins_edge = t[0];
        R.ins_long = t[1];
        spans = d_span.download(S);
        for (const PolSpan &s : spans)
            if (s.contig >= cs.size()) fail(HLMI_EINVAL, "%s: a row names a target that is no contig", who);    // (never)
    }
    polish_layout(cs, spans, who, L);

    // ---- CIGARs and rows ----------------------------------------------------------------------------------------------------------
    DBuf<PolRow> &d_rows = out.rows;
    DBuf<uint32_t> &d_ops = out.ops, d_cbase_of_crec;
    d_rows.alloc(std::max<size_t>(S, 1));
    d_ops.alloc(std::max<uint64_t>(n_ops, 1));
    if (weighted) out.quals.upload((const uint8_t *)rq.quals.data(), rq.quals.size());      // rs.off is DevReads::off of call.dQ
    if (S) {
        std::vector<uint32_t> cbase_of_crec(cs.size(), 0);
        for (size_t c = 0; c < cs.size(); ++c)
            if (L.rc[c]) cbase_of_crec[c] = L.cbase[L.slot_of_contig[c]];
        d_cbase_of_crec.upload(cbase_of_crec);
        std::vector<uint64_t> u_at;             // U / u in the reads (see pr_unvote_kernel)
        for (size_t p = rs.bases.find_first_of("Uu"); p != std::string::npos; p = rs.bases.find_first_of("Uu", p + 1)) u_at.push_back(p);
        DBuf<uint64_t> d_u_at;
        d_u_at.upload(u_at);
        KTimer kt("polish_rows");
        if (!u_at.empty())
            hipLaunchKernelGGL(pr_unvote_kernel, grid1(u_at.size()), dim3(WG), 0, stream(), call.dQ.codes(), d_u_at.p, u_at.size());
        hipLaunchKernelGGL(pr_write_kernel, grid1(S), dim3(WG), 0, stream(), rows.recs.p, idx.p, S, rows.ops_base, d_crec_of_rank.p,
                           d_qrec_of_rank.p, call.dQ.off.p, d_cbase_of_crec.p, (uint32_t)cs.size(), cig_off.p, cig_n.p, d_rows.p, d_ops.p);
        HIP_CHECK(hipGetLastError());
    }
    out.contig.upload((const uint8_t *)L.contigs.data(), L.contigs.size());
    out.cbase.upload(L.cbase);
    out.tiles.upload(L.tiles);
    PolCoreIn &c = out.core;
    c.rows = d_rows.p; c.n_rows = (uint32_t)S;
    c.ops = d_ops.p;
    c.reads = call.dQ.codes(); c.enc = READS_CODES;
    c.quals = weighted && !rq.quals.empty() ? out.quals.p : nullptr;
    c.contig = out.contig.p; c.n_contig = L.contigs.size();
    c.tiles = out.tiles.p; c.n_tiles = L.tiles.size();
    c.cbase = out.cbase.p; c.n_cbase = L.cbase.size();
}

void rows_from_reads(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const RowsRequest &q, PileupRows &R) {
    RowSelection &sel = R.dev;
    R.aligned = true;
    R.pc.path = q.pairs_paf;
    select_device_rows(contigs, reads, ao, q.min_len, q.min_iden, q.who, q.qc, q.pairs_paf ? &R.pc : nullptr, sel);
    const size_t S = R.n_sel = sel.n_sel;
    R.n_rows = sel.n_rows;
    R.t_dev = sel.t_dev;
    polish_check_weight_width(q.who.quals, q.qc, S);
    if (!q.spans_only) {
        refill_missing_quals(q, sel.rs, sel.rq);
        return device_rows_input(R, q.who.seqs, quals_travel(q));
    }

    // the spans: all that is read of the selected rows, and all that comes back of them for the layout
    R.d_spans.alloc(std::max<size_t>(S, 1));
    depth::depth_spans_from_rows(sel.rows.recs.p, sel.idx.p, S, sel.d_crec_of_rank.p, R.d_spans.p);
    const std::vector<PolSpan> spans = R.d_spans.download(S);
    for (const PolSpan &s : spans)
        if (s.contig >= sel.cs.size()) fail(HLMI_EINVAL, "%s: a row names a target that is no contig", q.who.seqs);      // (never)
    polish_layout(sel.cs, spans, q.who.seqs, R.L, false);
    if (S) R.upload_tiles();
}

void PileupRows::upload_tiles() {
    up.tiles.upload(L.tiles);
    up.cbase.upload(L.cbase);
    up.core.tiles = up.tiles.p; up.core.n_tiles = L.tiles.size();
    up.core.cbase = up.cbase.p; up.core.n_cbase = L.cbase.size();
}

std::vector<uint32_t> PileupRows::read_of_row() const {
    std::vector<uint32_t> r(n_sel);
    if (aligned) {
        r = ph::selected_query_ranks(dev.rows.recs.p, dev.idx.p, n_sel);
        for (uint32_t &q : r) q = q < dev.qrec_of_rank.size() ? dev.qrec_of_rank[q] : 0xffffffffu;
    } else {
        for (size_t i = 0; i < n_sel; ++i) r[i] = paf.sel[i].read;
    }
    return r;
}

}  // namespace pol

}  // namespace hlmi
