// polish_select.h - the row front of every pile-up call (hlmi_polish*, hlmi_depth, hlmi_variants, hlmi_phase, hlmi_haplotigs and
// their _reads forms): the row selection of include/hylight_mi.h (hlmi_polish_pairs: qname == tname, the read floor, the pair
// list, te == ts / min_len, min_iden, one row per read), the layout of the covered contigs and the selected rows as the device
// part's input.  An entry point fills a RowsRequest and calls one of two functions - rows_from_paf (polish_host.cpp) over a PAF
// file, rows_from_reads (polish_rows.hip) over the rows the overlapper leaves in HBM - and hands the PileupRows to its family's
// body, which does not know which of the two filled it.  The selection itself stays one function per kind of rows
// (select_paf_rows, select_device_rows), each called by its front alone.
#pragma once
#include <string>
#include <type_traits>
#include <vector>

#include "ava.h"
#include "common.h"
#include "paf_io.h"
#include "polish_internal.h"

namespace hlmi {
namespace pol {

// who names the entry point in the refusals; the older calls keep the names their messages always had
struct SelectNames {
    const char *seqs = "hlmi_polish";           // a sequence of 2^28 bases, a name twice, 2^31 contig bases (polish_layout)
    const char *quals = "hlmi_polish_q";        // polish_read_quals, polish_check_weight_width
    const char *list = "hlmi_polish_pairs";     // the pair list
    bool unique_names = false;                  // two records of one name in `contigs` or in `reads` are HLMI_EINVAL
};

// ---- over a PAF file ------------------------------------------------------------------------------------------------------------
struct PafSel {
    size_t line;            // 0-based PAF line
    uint32_t contig, read;  // records
};
struct PafSelection {
    SeqSet cs, rs;
    SeqQual rq;             // with qc
    PafText pt;
    std::vector<PafSel> sel;            // in the order (contig, ts, line)
};
// Reads the three files (and the list of pc), makes every refusal about the files, the rows and the list in hlmi_polish_pairs's
// order and selects.  qc == nullptr: no quality strings are read and no floor applies.  Sets qc's and pc's counters.
void select_paf_rows(const char *contigs, const char *reads, const char *paf, int min_len, double min_iden, const SelectNames &who,
                     PolQualCall *qc, PolPairCall *pc, PafSelection &out);

// ---- over the overlapper's rows in HBM ------------------------------------------------------------------------------------------
struct RowSelection {
    SeqSet cs, rs;
    SeqQual rq;             // with qc
    AvaPairCall call;
    AvaRows rows;
    std::vector<uint32_t> crec_of_rank, qrec_of_rank;      // name rank -> contig / read record (0xffffffff: none)
    DBuf<uint32_t> d_crec_of_rank, d_qrec_of_rank;         // uploaded when a row is selected
    DBuf<uint32_t> idx;                 // the selected rows' indices in rows.recs, in the order (contig, ts, line)
    size_t n_rows = 0, n_sel = 0;
    double t_dev = 0;                   // now_ms() where the device part began
};
// Reads both files, runs the overlapper and selects on the device: pr_facts_kernel, pr_winner_kernel, the flag-select, and the
// radix sort by contig record << 28 | ts.  Refusals: stub_oh >= 0, 2^28 bases, a name twice, 2^32 rows, the list's.
void select_device_rows(const char *contigs, const char *reads, const hlmi_ava_opts &ao, int min_len, double min_iden,
                        const SelectNames &who, PolQualCall *qc, PolPairCall *pc, RowSelection &out);

// ---- the selected rows, ready for a device part ---------------------------------------------------------------------------------
// what an entry point asks of the front
struct RowsRequest {
    SelectNames who;
    int min_len = 0;
    double min_iden = 0.0;
    PolQualCall *qc = nullptr;          // the _q part: floor, counters, and with qual_weight the quality bytes travel with the reads
    const char *pairs_paf = nullptr;    // nullptr: no list
    bool spans_only = false;            // hlmi_depth: no contig bytes, no PolRow, no CIGAR, no reads - spans, tiles and cbase only
    bool check_quals = false;           // rows_from_paf with no qc: read the quality strings all the same and refuse bad ones (no
                                        // floor, no weights).  rows_from_reads reads none without qc, whatever this says
    uint8_t quals_fill = 0;             // with qc, not 0: the quality bytes travel with the reads though no vote is weighted (no
                                        // polish_check_weight_width: that is qual_weight's), and a record without a quality
                                        // string travels as this byte, not as SeqQual's '!' (the variant calls' base floor)
};
// do the quality bytes go to the device?
inline bool quals_travel(const RowsRequest &q) { return q.qc && (q.qc->qual_weight || q.quals_fill); }
// quals_fill: the records without a quality string, refilled in place (the read floor was judged before: such a read is never low)
inline void refill_missing_quals(const RowsRequest &q, const SeqSet &rs, SeqQual &rq) {
    if (!q.qc || !q.quals_fill) return;
    for (size_t i = 0; i < rs.size() && i < rq.has_qual.size(); ++i)
        if (!rq.has_qual[i]) std::fill(rq.quals.begin() + rs.off[i], rq.quals.begin() + rs.off[i + 1], (char)q.quals_fill);
}
// the request of the calls that have one name in every refusal, no _q part and checked quality strings: all but hlmi_polish*
inline RowsRequest plain_request(const char *who, int min_len, double min_iden, const char *pairs_paf, bool spans_only = false) {
    return RowsRequest{SelectNames{who, who, who, true}, min_len, min_iden, nullptr, pairs_paf, spans_only, true};
}

// device memory behind a PolCoreIn (polish.hip fills it from a PolDevIn, polish_rows.hip where the overlapper's rows are)
struct PolUploaded {
    DBuf<uint8_t> contig, reads, quals;
    DBuf<PolRow> rows;
    DBuf<uint32_t> ops, cbase;
    DBuf<PolTile> tiles;
    PolCoreIn core;
};
void polish_upload(const PolDevIn &in, PolUploaded &up);        // core.min_cov is in.min_cov

struct PileupRows {
    bool aligned = false;               // filled by rows_from_reads
    PafSelection paf;                   // whichever of the two backs it
    RowSelection dev;
    const SeqSet &cs() const { return aligned ? dev.cs : paf.cs; }
    const SeqSet &rs() const { return aligned ? dev.rs : paf.rs; }
    PolLayout L;                        // L.contigs: the polished contigs' bytes (empty with spans_only)
    PolUploaded up;                     // up.core: min_cov is left to the body; with spans_only tiles and cbase alone are set
    DBuf<PolSpan> d_spans;              // with spans_only: the selected rows in their order
    size_t n_rows = 0, n_sel = 0;
    PolPairCall pc;                     // the list's counters; path == nullptr: no list was given
    uint64_t ins_edge = 0, ins_long = 0;
    double t_dev = 0;                   // where ms_device starts: before the uploads (PAF), where the overlapper starts (aligned)
    // The read record of every selected row (0xffffffff: none).  Over the overlapper's rows 4 bytes per row come down for it, so a
    // body asks only when it has a line to write.
    std::vector<uint32_t> read_of_row() const;
    void upload_tiles();                // with spans_only, of both fronts: L.tiles and L.cbase go up, up.core points at them
};
// Selection, polish_check_weight_width, polish_layout (its refusal names who.seqs), then the device part's input: PolRow, compact
// CIGARs (polish_rows.h), the aligned read stretches as ASCII, contig bytes, tiles and cbase, uploaded.
void rows_from_paf(const char *contigs, const char *reads, const char *paf, const RowsRequest &q, PileupRows &R);
// The same over the overlapper's rows: pr_count_kernel, the scan, polish_layout, pr_unvote_kernel, pr_write_kernel and the uploads
// of the layout; the reads stay the overlapper's codes (dev.call.dQ, which core points into).  With spans_only
// depth_spans_from_rows takes the place of the CIGAR kernels.
void rows_from_reads(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const RowsRequest &q, PileupRows &R);

// rows, contigs, rows_selected and, when a list was given, its three counters (hlmi_polish_stats has none: those of the _pairs
// calls reach hlmi_polish_pstats through capi.cpp)
template <class Stats>
void set_row_stats(const PileupRows &R, Stats *st) {
    st->rows = R.n_rows;
    st->contigs = R.cs().size();
    st->rows_selected = R.n_sel;
    if constexpr (!std::is_same_v<Stats, hlmi_polish_stats>) {
        if (!R.pc.path) return;
        st->pairs_listed = R.pc.pairs_listed;
        st->pairs_unknown = R.pc.pairs_unknown;
        st->rows_not_listed = R.pc.rows_not_listed;
    }
}

// The frame of an entry point: zeroed statistics, the stats of hlmi_last_stats_json reset, ms_total around everything.
template <class Stats, class Call>
void timed_call(Stats *st, bool reset_stats, Call &&call) {
    const double t_begin = now_ms();
    *st = Stats{};
    if (reset_stats) stat_reset();
    call();
    st->ms_total = now_ms() - t_begin;
}

}  // namespace pol
}  // namespace hlmi
