// polish_select.h - the row selection of include/hylight_mi.h (hlmi_polish_pairs: qname == tname, the read floor, the pair
// list, te == ts / min_len, min_iden, one row per read) as two functions, one per kind of entry point, so that every caller
// runs one implementation: the polisher (polish_host.cpp: polish_run, polish_rows.hip: polish_reads_run) and the depth call
// (depth_host.cpp) and the variant call (variants_host.cpp).  What a caller does with the selected rows is its own: spans
// alone (depth), or PolRow + compact CIGARs + reads, built by the second pair of functions below for the polisher and the
// variant call alike.
#pragma once
#include <string>
#include <vector>

#include "ava.h"
#include "common.h"
#include "paf_io.h"
#include "polish_internal.h"

namespace hlmi {
namespace pol {

// who names the entry point in the refusals; the older calls keep the names their messages always had
struct SelectNames {
    const char *seqs = "hlmi_polish";           // a sequence of 2^28 bases, a name twice
    const char *quals = "hlmi_polish_q";        // polish_read_quals
    const char *list = "hlmi_polish_pairs";     // the pair list
    bool unique_names = false;                  // two records of one name in `contigs` or in `reads` are HLMI_EINVAL
};

// ---- over a PAF file (hlmi_polish*, hlmi_depth) -------------------------------------------------------------------------------
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

// ---- over the overlapper's rows in HBM (hlmi_polish_reads*, hlmi_depth_reads) ------------------------------------------------
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

// ---- the selected rows as the device part's input (hlmi_polish*, hlmi_variants*) ----------------------------------------------
// PolRow, compact CIGARs (polish_rows.h), the aligned read stretches, tiles: what polish_core and variants_core read.  One
// implementation per kind of entry point, as for the selection.
//
// Over a PAF (polish_host.cpp): in.rows, in.ops, in.reads and, when weighted, in.quals from the selection, in its order; L is
// polish_layout's over the same rows.  Adds the rows' ins_edge and ins_long to the two counters.
void paf_rows_input(const PafSelection &S, const PolLayout &L, bool weighted, PolDevIn &in, uint64_t &ins_edge, uint64_t &ins_long);
// PolDevIn in device memory (polish.hip); core.min_cov is in.min_cov
struct PolUploaded {
    DBuf<uint8_t> contig, reads, quals;
    DBuf<PolRow> rows;
    DBuf<uint32_t> ops, cbase;
    DBuf<PolTile> tiles;
    PolCoreIn core;
};
void polish_upload(const PolDevIn &in, PolUploaded &up);

// Over the overlapper's rows (polish_rows.hip): pr_count_kernel, the scan, polish_layout (who: the entry point's name in its
// refusal; st: contigs_polished, may be nullptr), pr_unvote_kernel, pr_write_kernel and the uploads of the layout.  The reads
// stay the overlapper's codes (sel.call.dQ, which core points into); core.min_cov is left to the caller.
struct DeviceRowsInput {
    PolLayout L;
    DBuf<PolRow> rows;
    DBuf<uint32_t> ops, cbase;
    DBuf<PolTile> tiles;
    DBuf<uint8_t> contig, quals;
    PolCoreIn core;
    uint64_t ins_edge = 0, ins_long = 0;
};
void device_rows_input(const RowSelection &sel, const char *who, bool weighted, hlmi_polish_stats *st, DeviceRowsInput &out);

}  // namespace pol
}  // namespace hlmi
