// variants_qual_host_check.cpp - hylight_amd/csrc/variants_qual.h (whether a column passes the base floor, the D op's flank rule,
// the byte a FASTA record is filled with) held to literal answers, with the host compiler alone
// (tests/test_variants_qual_surface.py builds it with -fsanitize=address,undefined and runs it).  var_tile_kernel<QF>
// (variants.hip) compiles the same text.  The answers are the header's rules (include/hylight_mi.h: hlmi_variants_q) worked by
// hand; tests/test_variants_qual_model.py holds the model to the same literals.
#include <cstdio>
#include <vector>

#include "../../hylight_amd/csrc/variants_qual.h"

using namespace hlmi::var;

static int n_bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++n_bad; } \
    } while (0)

static std::vector<uint8_t> Q(std::initializer_list<int> phred) {
    std::vector<uint8_t> q;
    for (int p : phred) q.push_back((uint8_t)(33 + p));
    return q;
}

int main() {
    // a column at exactly the floor passes, one Phred below fails; floor 0 passes everything, floor 93 only '~'
    EXPECT(vq_byte_passes(33 + 10, 10) && !vq_byte_passes(33 + 9, 10) && vq_byte_passes(33 + 11, 10));
    EXPECT(vq_byte_passes(33, 0) && vq_byte_passes(126, 0) && !vq_byte_passes(33, 1) && vq_byte_passes(34, 1));
    EXPECT(vq_byte_passes(126, 93) && !vq_byte_passes(125, 93) && VQ_FLOOR_MAX == 93);
    // the FASTA fill passes every floor a call accepts
    for (uint32_t f = 0; f <= (uint32_t)VQ_FLOOR_MAX; ++f) EXPECT(vq_byte_passes(VQ_FASTA_FILL, f));
    EXPECT(VQ_FASTA_FILL >= 33 && VQ_FASTA_FILL <= 126);

    // the index: strand '+' reads the stretch forwards, strand '-' backwards (column i: read[qe - 1 - i])
    EXPECT(vq_index(8, 0, 0) == 0 && vq_index(8, 0, 7) == 7 && vq_index(8, 1, 0) == 7 && vq_index(8, 1, 7) == 0 && vq_index(1, 1, 0) == 0);

    {   // D between columns: the lower flank decides.  stretch Q: 30 30 5 30 30 30 30 30 (strand '+')
        const std::vector<uint8_t> q = Q({30, 30, 5, 30, 30, 30, 30, 30});
        EXPECT(vq_del_passes(q.data(), 8, 0, 1, 10));                // columns 0, 1: 30, 30
        EXPECT(!vq_del_passes(q.data(), 8, 0, 2, 10));               // columns 1, 2: the right flank is low
        EXPECT(!vq_del_passes(q.data(), 8, 0, 3, 10));               // columns 2, 3: the left flank is low
        EXPECT(vq_del_passes(q.data(), 8, 0, 4, 10));
        EXPECT(vq_del_passes(q.data(), 8, 0, 2, 5) && !vq_del_passes(q.data(), 8, 0, 2, 6));     // exactly at the floor
        // strand '-': column 2 is stretch byte 5 (Q30), column 5 is stretch byte 2 (Q5)
        EXPECT(vq_del_passes(q.data(), 8, 1, 2, 10) && vq_del_passes(q.data(), 8, 1, 3, 10));
        EXPECT(!vq_del_passes(q.data(), 8, 1, 5, 10) && !vq_del_passes(q.data(), 8, 1, 6, 10) && vq_del_passes(q.data(), 8, 1, 7, 10));
    }
    {   // a D as the first op has the column behind it alone, as the last op the one in front alone
        const std::vector<uint8_t> q = Q({3, 30, 30, 25});
        EXPECT(!vq_del_passes(q.data(), 4, 0, 0, 10) && vq_del_passes(q.data(), 4, 0, 0, 3));         // qc = 0: column 0 (Q3)
        EXPECT(vq_del_passes(q.data(), 4, 0, 4, 25) && !vq_del_passes(q.data(), 4, 0, 4, 26));        // qc = qn: column 3 (Q25)
        EXPECT(vq_del_passes(q.data(), 4, 1, 0, 25) && !vq_del_passes(q.data(), 4, 1, 0, 26));        // strand '-': column 0 is byte 3
        EXPECT(!vq_del_passes(q.data(), 4, 1, 4, 10));                                                // ... column 3 is byte 0
        // both flanks past the row's own columns (never: the host validates): no byte is read, the op passes
        EXPECT(vq_del_passes(q.data(), 4, 0, 5, 93));
    }
    {   // a row of D ops alone has no column at all: the op passes every floor, and no byte is read (a null stretch)
        EXPECT(vq_del_passes(nullptr, 0, 0, 0, 93) && vq_del_passes(nullptr, 0, 1, 0, 93));
    }
    {   // a stretch of one byte: both strands read byte 0, at qc 0 and at qc 1
        const std::vector<uint8_t> q = Q({7});
        EXPECT(vq_del_passes(q.data(), 1, 0, 0, 7) && !vq_del_passes(q.data(), 1, 0, 1, 8) && vq_del_passes(q.data(), 1, 1, 1, 7) &&
               !vq_del_passes(q.data(), 1, 1, 0, 8));
    }
    if (n_bad) return 1;
    printf("variants_qual_host_check: ok\n");
    return 0;
}
