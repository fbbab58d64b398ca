// polish_internal.h - what polish_host.cpp (validation, selection, text) and polish.hip (the votes and the bases) share.
// The rules are those of include/hylight_mi.h (hlmi_polish, hlmi_polish_q); tests/polish_model.py and
// tests/polish_qual_model.py restate them.
#pragma once
#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "common.h"
#include "paf_io.h"

namespace hlmi {
namespace pol {

constexpr int POLISH_TILE = 1024;       // contig positions per workgroup of the count pass (tests read this line)
constexpr int POLISH_INS_CAP = 16;      // longest insertion a row votes for (tests read this line)
constexpr uint32_t MAX_SEQ = 1u << 28;  // a position fits the 28 length bits of a CIGAR word

// decision of a position: 0..3 = A C G T, then
enum : uint8_t { SYM_DEL = 4, SYM_KEEP = 5 };

// A selected row.  Positions are the contig's own; `cbase` is where the contig starts in the concatenation of the polished
// contigs (the device's position space).  The read's aligned stretch read[qs, qe) lies at read_off in the uploaded reads.
struct PolRow {
    uint64_t read_off, cig_off;
    uint32_t cig_n, ts, te, qn;         // qn = qe - qs
    uint32_t rev, cbase;
};
// One tile of one contig: positions [t0, t0 + n_pos) and the rows [row_lo, row_hi) (sorted by contig, ts) that may overlap
// it - the first row whose end lies behind t0 to the last one that starts in front of the tile's end
struct PolTile {
    uint32_t t0, n_pos, row_lo, row_hi, cbase;
};

struct PolDevIn {
    std::string contigs, reads;         // concatenated: polished contigs; aligned read stretches
    std::string quals;                  // the stretches' quality bytes, parallel to `reads`; empty: every vote weighs 1
    std::vector<uint32_t> cbase;        // start of every polished contig in `contigs`, and the total behind the last
    std::vector<PolRow> rows;
    std::vector<uint32_t> ops;          // len << 4 | OP_*: zero-length ops dropped, neighbouring I ops merged
    std::vector<PolTile> tiles;
    int min_cov = 3;
};
struct PolDevOut {
    std::string bases;                  // the new contigs, concatenated
    std::vector<uint64_t> start;        // where each one starts in `bases`, and the total
    std::vector<uint8_t> sym;           // decision per position
    std::vector<uint32_t> open_pos;     // opened slots, ascending, and the length each one got
    std::vector<uint8_t> open_len;
};

// The device part over what is already in HBM: hlmi_polish reaches it behind polish_upload (rows_from_paf), hlmi_polish_reads
// (rows_from_reads) with the rows, compact CIGARs and reads where its own kernels and the overlapper left them.
enum ReadEnc : int { READS_ASCII = 0, READS_CODES = 1 };       // PolRow::read_off counts bytes of ASCII, or of DevReads::codes()
struct PolCoreIn {
    const PolRow *rows = nullptr;
    uint32_t n_rows = 0;
    const uint32_t *ops = nullptr;
    const uint8_t *reads = nullptr;
    const uint8_t *quals = nullptr;     // quality bytes (33..126), indexed exactly like `reads` by PolRow::read_off; nullptr: unweighted
    ReadEnc enc = READS_ASCII;
    const uint8_t *contig = nullptr;    // the polished contigs side by side, ASCII as in the file (their case reaches the output)
    size_t n_contig = 0;
    const PolTile *tiles = nullptr;
    size_t n_tiles = 0;
    const uint32_t *cbase = nullptr;    // PolDevIn::cbase
    size_t n_cbase = 0;
    int min_cov = 3;
};
void polish_core(const PolCoreIn &in, PolDevOut &out);

// polish_core behind its count pass, over any position space: n positions with their contig bytes, decisions and slot flags
// (device memory), the start of every output record in it (cbase, n_cbase entries, the total last).  Opened slots get their
// index; votes(0, ...) adds every inserting row's length vote to len_cnt[slot * POLISH_INS_CAP + len - 1], the lengths are
// decided, votes(1, ...) adds the base votes to base_cnt[(slot * POLISH_INS_CAP + j) * 4 + base] where win_len[slot] is the
// row's length; then output lengths, the scan and the bytes.  slots_timer: the kernel timer's name of the slot passes.
struct PolTailIn {
    const uint8_t *contig;
    size_t n;
    const DBuf<uint8_t> *sym, *open;
    const uint32_t *cbase;
    size_t n_cbase;
    const char *slots_timer;
};
using PolSlotVotes = std::function<void(int mode, const uint32_t *slot_of, const uint8_t *win_len, uint32_t *len_cnt, uint32_t *base_cnt)>;
void polish_tail(const PolTailIn &in, const PolSlotVotes &votes, PolDevOut &out);
constexpr uint32_t POLISH_NO_SLOT = 0xffffffffu;        // slot_of of a position whose slot stays shut
// polish_core's slot passes alone, for a caller with slots of its own (hlmi_variants_ins: its insertion sites): the n slots at the
// ascending positions d_pos get their index in d_slot_of (one entry per position of in.contig, POLISH_NO_SLOT everywhere), every
// row of `in` votes as in polish_core - lengths into d_len_cnt, the winning lengths into d_win_len (a tie: the smaller), bases
// into d_base_cnt, laid out as polish_tail's votes are.  The caller zeroes the counters.  in.quals != nullptr: weighted.
void polish_slot_votes(const PolCoreIn &in, const uint32_t *d_pos, size_t n, uint32_t *d_slot_of, uint8_t *d_win_len, uint32_t *d_len_cnt,
                       uint32_t *d_base_cnt);

// ---- what the pile-up calls do on the host around the device part (polish_host.cpp) ----------------------------------------
// a selected row as the layout sees it: contig record, [ts, te); in the order (contig, ts, line)
struct PolSpan {
    uint32_t contig, ts, te;
};
struct PolLayout {
    std::vector<uint32_t> rc;               // selected rows per contig record (RC:i:)
    std::vector<uint32_t> slot_of_contig;   // contig record -> its place among the polished ones
    std::vector<uint32_t> cbase;            // PolDevIn::cbase
    std::string contigs;                    // PolDevIn::contigs
    std::vector<PolTile> tiles;
};
// who: the entry point's name for the refusal of 2^31 contig bases.  The polished contigs number L.cbase.size() - 1.  with_bytes
// false: L.contigs stays empty (the depth call reads no contig byte)
void polish_layout(const SeqSet &cs, const std::vector<PolSpan> &sel, const char *who, PolLayout &L, bool with_bytes = true);

// The decisions of one record: a polished contig of `len` positions whose bytes are `contig`, on the side whose decisions and
// slots begin at g0 in out.sym / out.open_pos (hlmi_polish: the contig's cbase; hlmi_haplotigs: side * n_contig behind it).
// Adds its deleted and substituted positions, opened slots and their bases to st; -> the positions with a decision (XC:f:).
template <class Stats>
uint64_t count_decisions(const PolDevOut &out, size_t g0, const char *contig, uint32_t len, Stats *st) {
    uint64_t covered = 0;
    for (uint32_t p = 0; p < len; ++p) {
        const uint8_t d = out.sym[g0 + p];
        if (d == SYM_KEEP) continue;
        ++covered;
        if (d == SYM_DEL) ++st->deleted;
        else if ("ACGT"[d & 3] != (char)((unsigned char)contig[p] & 0xdfu)) ++st->substituted;
    }
    const auto s0 = std::lower_bound(out.open_pos.begin(), out.open_pos.end(), (uint32_t)g0);
    const auto s1 = std::lower_bound(s0, out.open_pos.end(), (uint32_t)(g0 + len));
    st->slots_opened += (uint64_t)(s1 - s0);
    for (auto it = s0; it != s1; ++it) st->inserted_bases += out.open_len[it - out.open_pos.begin()];
    return covered;
}

// The quality part of a _q call (nullptr: hlmi_polish / hlmi_polish_reads as they were).  In: the two options; out: the two
// counters of hlmi_polish_qstats.
struct PolQualCall {
    int qual_weight = 0;
    double min_avg_qual = 0.0;
    uint64_t reads_with_qual = 0, rows_low_qual = 0;
};
// Reads `reads` with its quality strings and judges them (seq_scan.h: quality_facts): a string of another length than its
// bases or a byte outside 33..126 is HLMI_EINVAL naming the record; sets qc.reads_with_qual; -> per record "this read is low"
// (empty when min_avg_qual == 0.0).  Both entry points start with it.
std::vector<uint8_t> polish_read_quals(const char *who, const char *reads, double min_avg_qual, SeqSet &rs, SeqQual &rq, PolQualCall &qc);
// qual_weight = 1: rows_selected x 93 must fit the 32-bit weight sums
void polish_check_weight_width(const char *who, const PolQualCall *qc, uint64_t rows_selected);

// The pair list of a _pairs call (nullptr: no list, every row may vote).  In: the list's path; out: the three counters of
// hlmi_polish_pstats.  The list's text is scanned by pair_list.h in hlmi_polish_pairs and by polish_pairs.hip in the fused call.
struct PolPairCall {
    const char *path = nullptr;
    uint64_t pairs_listed = 0, pairs_unknown = 0, rows_not_listed = 0;
};
// hlmi_polish_reads_pairs (polish_pairs.hip): the list parsed on the device against the call's name ranks (AvaPairCall::
// name_of_rank, the qid / tid space of the overlapper's rows) -> the distinct keys rank_a << 32 | rank_b of the listed pairs in
// both orders, ascending (at least one element is allocated: a null pointer means "no list" to pr_facts_kernel).  A line with
// fewer than 6 fields is HLMI_EINVAL naming `who` and the line.  Sets pc.pairs_listed and pc.pairs_unknown.
struct PairKeys {
    DBuf<uint64_t> keys;
    size_t n = 0;
};
void pair_keys_device(const char *who, const std::vector<std::string> &name_of_rank, PolPairCall &pc, PairKeys &out);

}  // namespace pol

// qc, pc: the _q and _pairs parts (capi.cpp), nullptr without; pc's counters are set when the rows are there
void polish_run(const char *contigs, const char *reads, const char *paf, const hlmi_polish_opts &o, const char *out_fa,
                hlmi_polish_stats *st, pol::PolQualCall *qc = nullptr, pol::PolPairCall *pc = nullptr);
// hlmi_polish_reads: the overlapper's rows selected, ordered and compacted where they are (polish_rows.hip)
void polish_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_polish_opts &po,
                      const char *out_fa, hlmi_polish_stats *st, pol::PolQualCall *qc = nullptr, pol::PolPairCall *pc = nullptr);

}  // namespace hlmi
