// polish_internal.h - what polish_host.cpp (validation, selection, text) and polish.hip (the votes and the bases) share.
// The rules are those of include/hylight_mi.h (hlmi_polish); tests/polish_model.py restates them.
#pragma once
#include <string>
#include <vector>

#include "common.h"

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
void polish_device(const PolDevIn &in, PolDevOut &out);

}  // namespace pol

void polish_run(const char *contigs, const char *reads, const char *paf, const hlmi_polish_opts &o, const char *out_fa,
                hlmi_polish_stats *st);

}  // namespace hlmi
