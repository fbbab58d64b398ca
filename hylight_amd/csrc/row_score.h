// row_score.h - the three scores of a final row (filter_overlap_slr2.py:113,138-146), the one definition for row_text.hip and
// for paf_io.cpp:format_scored_row:
//   score  = 0.4 mc / ((ql + tl) / 2) + 0.6 mc / len,   score2 = 1 - sum_of_X_digits / mc,   score3 = mc / len
// as IEEE doubles in the reference's evaluation order (whoever compiles this file passes -ffp-contract=off; double division is
// correctly rounded on gfx950 as on the host), each as the integer its "%.4f" shows (dec_text.h), the `float(score2) < iden`
// test (slr2:146) on those four decimals, and column 12 as sort_scored_lines' key.  Checked by tests/capi/dec_text_host_check.cpp.
#pragma once
#include <cstdint>

#include "dec_text.h"

namespace hlmi {
constexpr uint32_t SCORE_KEY_LIMIT = 1u << 22;                // 419.4304: column 12 below it is its own sort key
enum : int {
    SCORE_DROPPED = 0,        // float(score2) < iden: the row is not written
    SCORE_KEPT = 1,
    SCORE_GENERAL = 2,        // a score outside fixed4_q's range (mc or len of 0, more X digits than matches): the general formatter
};
struct RowScore {
    uint64_t q1, q2, q3;      // score, score2, score3 x 10^4: put_fixed4 writes columns 12 to 14 from them
    uint32_t key;             // q1 below SCORE_KEY_LIMIT, else 0xffffffff
};
// -> SCORE_*; s is complete unless SCORE_GENERAL comes back
HLMI_HD int row_score(uint32_t nmatch, uint32_t blen, uint32_t qlen, uint32_t tlen, uint32_t xsum, double iden, RowScore &s) {
    const double mc = (double)nmatch, ln = (double)blen;
    const double mlen = (double)((uint64_t)qlen + tlen) / 2.0;
    const double t1 = mc / mlen, t2 = mc / ln;
    const double a = 0.4 * t1, b = 0.6 * t2;
    const double score = a + b;
    const double mis = (double)xsum / mc;
    const double score2 = 1.0 - mis;
    if (!fixed4_q(score, s.q1) || !fixed4_q(score2, s.q2) || !fixed4_q(t2, s.q3)) return SCORE_GENERAL;
    if (s.q2 >= (1ull << 53)) return SCORE_GENERAL;
    s.key = s.q1 < (uint64_t)SCORE_KEY_LIMIT ? (uint32_t)s.q1 : 0xffffffffu;
    const double shown = (double)s.q2 / 10000.0;             // float("0.9876"): the correctly rounded 9876 / 10^4
    return shown < iden ? SCORE_DROPPED : SCORE_KEPT;
}
}  // namespace hlmi
