// variants_qual.h - the base-quality floor of hlmi_variants_q and its _reads and _ins forms (include/hylight_mi.h): whether a
// column's vote passes, the D op's flank rule, and the byte a record without a quality string is filled with.  var_tile_kernel<QF>
// (variants.hip) and tests/capi/variants_qual_host_check.cpp compile this one text; nothing of HIP's is included (hd.h).
// A floor and no weight: min_alt, depth, alt_count and alt_frac are counts of reads and stay counts.
#pragma once
#include <cstdint>

#include "hd.h"

namespace hlmi {
namespace var {

constexpr int VQ_FLOOR_MAX = 93;                // 126 - 33: the highest Phred a quality byte can state
// What the row front writes where a record has no quality string (FASTA): Phred 93 passes every floor of 0..93.  SeqQual's own
// fill, '!', is Phred 0 - right for the polisher's weights (max(1, 0) = 1), but under a floor it would silence the whole read.
constexpr uint8_t VQ_FASTA_FILL = 126;

// q = byte - 33; an = / X column whose base is A C G T passes iff q >= min_base_qual (bytes are 33..126: validated on the host)
HLMI_HD bool vq_byte_passes(uint32_t byte, uint32_t min_base_qual) { return byte >= min_base_qual + 33u; }

// where alignment column `col` of a row of qn query columns lies in the row's stretch of the read: strand '-' reads it backwards
// (column i has the quality of read[qe - 1 - i]).  col < qn -> the index lies in [0, qn)
HLMI_HD uint32_t vq_index(uint32_t qn, uint32_t rev, uint32_t col) { return rev ? qn - 1u - col : col; }

// A D op whose first query column behind it is qc: its q is the lower q of query columns qc - 1 and qc, of those inside [0, qn);
// with neither present the op passes.  `quals`: the row's stretch (qn bytes).  All columns of the op pass or fail together.
HLMI_HD bool vq_del_passes(const uint8_t *quals, uint32_t qn, uint32_t rev, uint32_t qc, uint32_t min_base_qual) {
    uint32_t lo = 0xffffffffu;
    if (qc >= 1u && qc - 1u < qn) lo = quals[vq_index(qn, rev, qc - 1u)];
    if (qc < qn) {
        const uint32_t b = quals[vq_index(qn, rev, qc)];
        lo = b < lo ? b : lo;
    }
    return lo == 0xffffffffu || vq_byte_passes(lo, min_base_qual);
}

}  // namespace var
}  // namespace hlmi
