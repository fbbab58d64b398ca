// align_score_setup.h - what the alignment pass derives from the scoring options alone: which kernel forms may run and
// which certificates of classify_kernel hold for these constants.  Pure host arithmetic (no device, no runtime): the
// answers of the test hooks are passed in, so tests/capi/align_setup_host_check.cpp can hold it to literal values.
#pragma once
#include <algorithm>

#include "../../include/hylight_mi.h"

namespace hlmi {

// spec constants this header needs (ava.h has them under the same names without the prefix; ava_align.hip asserts equality)
constexpr int SETUP_BLOCK_MAX = 256, SETUP_NARROW_W = 16, SETUP_EXT_MAX = 256;
constexpr int SETUP_LONG_ROWS_EXTRA = 136;      // long_rows_cap(o) - ext_rows(o)
// (the rows test below is long_rows_cap(o) > 32 000 written out: it must follow ext_rows / long_rows_cap of ava.h)
constexpr int SETUP_LONG_ROWS_MAX = 32000;

struct AlignScoreHooks {            // true: the hook of that name is set
    bool narrow_unpacked = false;   // HLMI_NARROW_UNPACKED
    bool stub_full_rows = false;    // HLMI_STUB_FULL_ROWS
    bool no_gap1_cert = false, no_gap2_cert = false, no_shift_cert = false, no_ext_cert = false, no_one_piece_cert = false;
    bool no_suffix_trim = false;    // HLMI_NO_SUFFIX_TRIM
};
enum AlignScoreError {
    ALIGN_SCORE_OK = 0,
    ALIGN_SCORE_GAP2_CHEAP,         // the second piece of the gap cost is the cheaper one below NARROW_W bases
    ALIGN_SCORE_ROWS                // max_gap asks for tasks of more than 32 000 rows
};
struct AlignScoreSetup {
    AlignScoreError error;
    bool packed;            // packed form of the near-diagonal DP (two tasks per lane, 16-bit scores)
    bool bare;              // stub rule, second half: the tasks of stub candidates report scores only
    bool ext_all_long;      // every extension runs in align_long_kernel (see below)
    int go2, ge2;           // second piece of the gap cost (0, 0: one piece)
    int kmax, kgap1, kgap2, kshift, kext_plain, kext_bonus, trim_ok, one_ok;      // AlignArgs fields of the same names
};

inline AlignScoreSetup align_score_setup(const hlmi_ava_opts &o, const AlignScoreHooks &h) {
    AlignScoreSetup s{};
    s.go2 = o.gap_open2 > 0 ? o.gap_open2 : 0;
    s.ge2 = o.gap_open2 > 0 ? o.gap_ext2 : 0;
    // LONG tasks: a chain link spans at most max_gap bases and an extension ext_rows(o) rows
    if (std::max(o.max_gap, SETUP_EXT_MAX) + SETUP_LONG_ROWS_EXTRA > SETUP_LONG_ROWS_MAX) s.error = ALIGN_SCORE_ROWS;
    // the 16-diagonal kernels (gaps of at most 15 bases) know the first piece only
    else if (s.go2 && s.go2 + s.ge2 * (SETUP_NARROW_W - 1) < o.gap_open + o.gap_ext * (SETUP_NARROW_W - 1)) s.error = ALIGN_SCORE_GAP2_CHEAP;
    // packed form: block scores must stay within +-4096 of the bias
    const int worst = std::max(std::max(o.match, o.mismatch), std::max(o.ambi, o.gap_open + o.gap_ext));
    s.packed = worst > 0 && (long long)worst * (SETUP_BLOCK_MAX + SETUP_NARROW_W + 2) <= 4000 && o.match >= 0 && o.mismatch >= 0 &&
               o.ambi >= 0 && o.gap_open >= 0 && o.gap_ext >= 0 && !h.narrow_unpacked;
    // nobody reads the content of a stub candidate's row (score-only instances of the packed and the 64-diagonal kernel;
    // HLMI_STUB_FULL_ROWS keeps the candidates' CIGARs: test hook)
    s.bare = o.stub_oh >= 0 && s.packed && !h.stub_full_rows;
    // An extension of <= EXT_MAX rows runs in the 64-diagonal kernels, which know no z-drop: it cannot matter there when a
    // drop of more than zdrop (at most D per row, D = the dearest single step) plus the climb back above the old best cell
    // (at most `match` per row) need more rows than EXT_MAX - otherwise every extension is a LONG task.
    if (o.zdrop > 0) {
        const int D = std::max(std::max(o.mismatch, o.ambi), o.gap_open + o.gap_ext);
        const int rows_down = D > 0 ? (o.zdrop + D - 1) / D : SETUP_EXT_MAX;
        // (the best cell is ranked with the end bonus: a row that reaches the query end counts end_bonus more)
        s.ext_all_long = (long long)o.match * (SETUP_EXT_MAX - rows_down) + std::max(o.end_bonus, 0) > o.zdrop;
    }
    // largest k with k*(match+mismatch) < match + 2*(open+ext), capped at 3 (7 runs)
    const int U = o.match + o.mismatch, T = o.match + 2 * (o.gap_open + o.gap_ext);
    s.kmax = U > 0 && T > 0 ? std::min(3, (T - 1) / U) : 0;
    if (o.match <= 0 || o.gap_open < 0 || o.gap_ext <= 0) s.kmax = -1;   // proof needs sane scores
    // fifth certificate: one substitution gains less than a further inserted + deleted base costs
    s.kgap1 = s.kmax >= 0 && U < o.gap_open + 2 * o.gap_ext + o.match && !h.no_gap1_cert ? 1 : 0;
    // seventh certificate: see classify_kernel (c(L) = the cheaper piece's cost of a gap of L bases)
    auto c = [&](int L) { int v = o.gap_open + o.gap_ext * L; if (o.gap_open2 > 0) v = std::min(v, o.gap_open2 + o.gap_ext2 * L); return v; };
    s.kgap2 = s.kgap1 && U < o.match + c(2) && 2 * U < o.match + 2 * c(1) && 2 * U < 2 * o.match + c(2) + c(3) - c(1) &&
              c(2) == o.gap_open + 2 * o.gap_ext && c(1) == o.gap_open + o.gap_ext && !h.no_gap2_cert ? 1 : 0;
    // fourth certificate: with k = kmax + 1 substitutions the only gapped paths that reach the diagonal's score
    // have one inserted + one deleted base and no mismatch; paths with a further gap base pair lose another
    // match + 2 ext, paths with a further gap another open + ext + match (three positions fit the run buffer)
    const int k = s.kmax + 1;
    s.kshift = s.kmax >= 0 && k <= 3 && k * U > T && k * U < T + o.match + std::min(2 * o.gap_ext, o.gap_open + o.gap_ext) &&
               !h.no_shift_cert ? 1 : 0;
    s.trim_ok = h.no_suffix_trim ? 0 : 1;
    s.one_ok = h.no_one_piece_cert ? 0 : 1;
    // sixth certificate (classify_kernel: extensions with one or two substitutions); G = cheapest one-base gap
    int G = o.gap_open + o.gap_ext;
    if (s.go2 > 0) G = std::min(G, s.go2 + s.ge2);
    const bool sane = s.kmax >= 0 && o.match > 0 && o.mismatch >= 0 && !h.no_ext_cert;
    s.kext_plain = sane && G >= U && U < 2 * G + o.match ? 1 : 0;
    for (int kk = 1; kk <= 2; ++kk)
        if (sane && o.end_bonus > 0 && kk * U < G && kk * U < o.end_bonus + o.match && kk * U < 2 * G + o.match) s.kext_bonus = kk;
    return s;
}

}  // namespace hlmi
