// polish_select.h - the row selection of include/hylight_mi.h (hlmi_polish_pairs: qname == tname, the read floor, the pair
// list, te == ts / min_len, min_iden, one row per read) as two functions, one per kind of entry point, so that every caller
// runs one implementation: the polisher (polish_host.cpp: polish_run, polish_rows.hip: polish_reads_run) and the depth call
// (depth_host.cpp).  What a caller does with the selected rows - compact CIGARs and votes, or spans alone - is its own.
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

}  // namespace pol
}  // namespace hlmi
