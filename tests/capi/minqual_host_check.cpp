// Stand-alone check of the consensus tables per minQual - hylight_amd/csrc/vq_superread.cpp, pure host code -, meant to be built
// with the host sanitizers and run on its own, as tests/capi/clique_host_check.cpp is - no GPU, no Python:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
//       -I<rocm>/include tests/capi/minqual_host_check.cpp hylight_amd/csrc/vq_superread.cpp -o minqual_host_check
//   ./minqual_host_check
// For minQual 0, 0.5, 0.9 and 1 it builds the tables and holds every cell of every section to vq_consensus_pos itself, called
// for every pair of bases the cell stands for and decoded the way the kernels decode it (vqm::pair_base is device code; its rule
// is restated here).  With glibc's libm the build refuses minQual 1 - twice one base at Q61 / Q93 is N for C and G and the base
// for A and T, by the last bit of a quotient -; the program then shows that with vq_consensus_pos alone and accepts the refusal.  Then what the tables must look like: codes 3 and 4 of T_DIFF where they belong at minQual 0, none at 0.9,
// one table per value, -0.0 the same entry as 0.0, and the values outside [0, 1] refused.  Exit status 0 when everything holds.
#include <cmath>
#include <cstdio>
#include <limits>

#include "../../hylight_amd/csrc/vq_internal.h"

using namespace hlmi;
using namespace hlmi::vqm;

static int bad = 0;
static void expect(bool ok, const char *what, double mq, int q1 = -1, int q2 = -1) {
    if (!ok && ++bad <= 20) printf("FAILED at minQual %g (Q%d, Q%d): %s\n", mq, q1, q2, what);
}

static int rank_atcg(int c) { return c == 0 ? 0 : c == 3 ? 1 : c == 1 ? 2 : 3; }      // A C G T = 0 .. 3 -> place in A, T, C, G

// the base and quality a two-base cell gives for bases c1, c2: the select of merge_kernel and pile_kernel
static uint16_t decode(uint16_t cell, int c1, int c2) {
    const char B[5] = "ACGT";
    const int act = cell >> 8;
    char other = 0;
    for (int c : {2, 1, 3, 0})                   // (the last one kept is the first of A, T, C, G)
        if (c != c1 && c != c2) other = B[c];
    const char b = act == 0 ? 'N' : act == 1 ? B[c1] : act == 2 ? B[c2] : act == 4 ? other : rank_atcg(c2) < rank_atcg(c1) ? B[c2] : B[c1];
    return (uint16_t)((b << 8) | (cell & 0xff));
}

// true when one (q1, q2) gives twice one base a different class of answer - N, that base, another - for different bases: the
// reference's own answer then depends on the order of the four terms of total_prob, and no table by class can hold it
static bool same_base_cells_disagree(double mq) {
    for (int q1 = 0; q1 < NQ; ++q1)
        for (int q2 = 0; q2 < NQ; ++q2) {
            const int ph[2] = {q1, q2};
            int first = -1;
            for (const char *nuc : {"AA", "CC", "GG", "TT"}) {
                const char b = (char)(vq_consensus_pos(nuc, ph, 2, mq) >> 8);
                const int cls = b == 'N' ? 0 : b == nuc[0] ? 1 : 2;
                if (first < 0) first = cls;
                if (cls != first) return true;
            }
        }
    return false;
}

static void check_tables(double mq) {
    const std::vector<uint16_t> *built = nullptr;
    int code = 0;
    try { built = &vq_consensus_tables(mq); } catch (const Error &e) { code = e.code; }
    if (!built) {
        // Only at minQual 1 may the build refuse: 1 - p_incorrect < 1 is then decided by the last bit of max_prob / total_prob.
        // The refusal must be HLMI_EINVAL and must be true: shown here with vq_consensus_pos alone.
        const bool true_refusal = code == HLMI_EINVAL && mq == 1.0 && same_base_cells_disagree(mq);
        printf("minQual %-4g refused (%d): the answer depends on the bases' identity: %s\n", mq, code, true_refusal ? "confirmed" : "NOT confirmed");
        expect(true_refusal, "a refused table build", mq);
        return;
    }
    expect(!same_base_cells_disagree(mq), "tables were built though the classes do not hold", mq);
    const std::vector<uint16_t> &t = *built;
    expect(t.size() == (size_t)T_ALL, "table size", mq);
    if (t.size() != (size_t)T_ALL) return;
    const char B[6] = "ACGTN";
    int threes = 0, threes_off_diagonal = 0, fours = 0, fours_high = 0;
    for (int q1 = 0; q1 < NQ; ++q1) {
        for (int c = 0; c < 5; ++c) expect(t[T_SINGLE + c * NQ + q1] == vq_consensus_pos(&B[c], &q1, 1, mq), "T_SINGLE", mq, q1);
        for (int q2 = 0; q2 < NQ; ++q2) {
            const int ph[2] = {q1, q2}, hp[2] = {q2, q1};
            for (int c = 0; c < 4; ++c) {
                const char with_n[2] = {B[c], 'N'}, n_with[2] = {'N', B[c]};
                expect(t[T_WITH_N + c * NQ + q1] == vq_consensus_pos(with_n, ph, 2, mq), "T_WITH_N, the base first", mq, q1, q2);
                expect(t[T_WITH_N + c * NQ + q1] == vq_consensus_pos(n_with, hp, 2, mq), "T_WITH_N, the N first", mq, q1, q2);
            }
            expect(vq_consensus_pos("NN", ph, 2, mq) == (uint16_t)(('N' << 8) | '$'), "N against N", mq, q1, q2);
            const uint16_t same = t[T_SAME + q1 * NQ + q2], diff = t[T_DIFF + q1 * NQ + q2];
            expect((same >> 8) <= 1 || (same >> 8) == 4, "T_SAME holds 0, 1 or 4", mq, q1, q2);
            expect((diff >> 8) <= 4, "T_DIFF holds 0 .. 4", mq, q1, q2);
            if ((diff >> 8) == 3) { ++threes; threes_off_diagonal += q1 != q2; }
            if ((diff >> 8) == 4) { ++fours; fours_high += q1 > 1 || q2 > 1; }
            for (int c1 = 0; c1 < 4; ++c1)
                for (int c2 = 0; c2 < 4; ++c2) {
                    const char nuc[2] = {B[c1], B[c2]};
                    expect(decode(c1 == c2 ? same : diff, c1, c2) == vq_consensus_pos(nuc, ph, 2, mq), "a two-base cell", mq, q1, q2);
                }
        }
    }
    printf("minQual %-4g %5d cells of T_DIFF hold code 3 (%d off the diagonal), %d hold code 4\n", mq, threes, threes_off_diagonal, fours);
    // a base is more likely wrong than right below Q1.25: both are in the four cells of Q0 / Q1, and there no read base wins
    if (mq == 0.0) expect(threes == NQ - 2 && threes_off_diagonal == 0 && fours == 4 && fours_high == 0,
                          "minQual 0: code 4 for Q0 / Q1 against Q0 / Q1, code 3 on the rest of the diagonal, nowhere else", mq);
    // an even split of two read bases leaves each less than 1/2 (the two others take the rest): N.  At Q0 against Q0 the read
    // bases score nothing and the two others split evenly: exactly 1/2, which is not below minQual 1/2
    if (mq == 0.5) expect(threes == 0 && fours == 1 && (t[T_DIFF] >> 8) == 4, "minQual 0.5: no code 3, code 4 at Q0 / Q0 alone", mq);
    if (mq > 0.5) expect(threes == 0 && fours == 0, "minQual above 0.5: no code 3 or 4", mq);
}

static void check_values() {
    // the hand-worked cases of tests/test_vq_minqual_model.py, on the host's own evaluation
    const int q40[2] = {40, 40}, q40_20[2] = {40, 20};
    auto col = [](char b, char q) { return (uint16_t)((b << 8) | q); };
    expect(vq_consensus_pos("AG", q40, 2, 0.0) == col('A', '$') && vq_consensus_pos("GA", q40, 2, 0.0) == col('A', '$'), "A / G tie", 0);
    expect(vq_consensus_pos("CT", q40, 2, 0.0) == col('T', '$') && vq_consensus_pos("TC", q40, 2, 0.0) == col('T', '$'), "C / T tie", 0);
    expect(vq_consensus_pos("CG", q40, 2, 0.0) == col('C', '$') && vq_consensus_pos("GC", q40, 2, 0.0) == col('C', '$'), "C / G tie", 0);
    expect(vq_consensus_pos("TG", q40, 2, 0.0) == col('T', '$') && vq_consensus_pos("GT", q40, 2, 0.0) == col('T', '$'), "T / G tie", 0);
    expect((vq_consensus_pos("AG", q40_20, 2, 0.0) >> 8) == 'A', "A/Q40 against G/Q20", 0);
    expect(vq_consensus_pos("AG", q40, 2) == col('N', '$') && vq_consensus_pos("AG", q40, 2, VQ_MIN_QUAL) == col('N', '$'), "the default is 0.9", 0.9);
    expect(vq_consensus_pos("NN", q40, 2, 0.0) == col('N', '$'), "N against N at minQual 0", 0);
    for (int q = 0; q < NQ; ++q)
        for (const char *b : {"A", "C", "G", "T", "N"})
            expect(vq_consensus_pos(b, &q, 1, 0.0) == vq_consensus_pos(b, &q, 1, 0.9), "one base does not read minQual", 0, q);
}

static void check_cache_and_bounds() {
    const std::vector<uint16_t> *a = &vq_consensus_tables(0.0), *b = &vq_consensus_tables(0.9);
    expect(a != b && *a != *b, "two values, two tables", 0);
    expect(&vq_consensus_tables(0.0) == a && &vq_consensus_tables(-0.0) == a && &vq_consensus_tables(0.9) == b, "built once per value", 0);
    expect(&vq_consensus_tables(0.5) != a && &vq_consensus_tables(0.0) == a, "an entry stays where it is when another is added", 0);
    for (double v : {-0.1, 1.1, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
        int code = 0;
        try { vq_check_min_qual(v, "check"); } catch (const Error &e) { code = e.code; }
        expect(code == HLMI_EINVAL, "vq_check_min_qual refuses", v);
        code = 0;
        try { vq_consensus_tables(v); } catch (const Error &e) { code = e.code; }
        expect(code == HLMI_EINVAL, "vq_consensus_tables refuses", v);
    }
    for (double v : {0.0, -0.0, 0.5, 1.0}) {
        int code = 0;
        try { vq_check_min_qual(v, "check"); } catch (const Error &e) { code = e.code; }
        expect(code == 0, "vq_check_min_qual accepts", v);
    }
}

int main() {
    for (double mq : {0.0, 0.5, 0.9, 1.0}) check_tables(mq);
    check_values();
    check_cache_and_bounds();
    printf("minqual_host_check: %d problems\n", bad);
    return bad ? 1 : 0;
}
