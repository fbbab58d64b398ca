// Host check of hylight_amd/csrc/align_score_setup.h: what the alignment pass derives from the scoring options - kernel forms
// and certificates - held to literal answers.  Plain C++, no device: built by tests/test_align_setup.py, also under the address
// and undefined-behaviour sanitizers.
//
// The long-constant row by hand (match 2, mismatch 4, open 4, ext 2, ambi 1, second piece 24 + 1 L, z-drop 400, no end bonus):
//   packed    dearest step max(2, 4, 1, 4 + 2) = 6; 6 * (256 + 16 + 2) = 1644 <= 4000: yes
//   all LONG  a drop of 400 takes ceil(400 / 6) = 67 rows, the climb back 2 per row: 2 * (256 - 67) = 378 is not > 400: no
//   kmax      U = 2 + 4 = 6, T = 2 + 2 * 6 = 14: largest k with 6 k < 14 is 2
//   fifth     6 < 4 + 2 * 2 + 2 = 10: yes
//   seventh   c(1) = 6, c(2) = 8, c(3) = 10 (the first piece is the cheaper one up to 20 bases): 6 < 2 + 8, 12 < 2 + 12, 12 < 4 + 8 + 10 - 6: yes
//   fourth    k = 3: 18 > 14 and 18 < 14 + 2 + min(4, 6) = 20: yes
//   sixth     G = 6 >= U = 6 and 6 < 12 + 2: plain yes; no end bonus: bonus form 0
// and the short one (match 4, mismatch 2, open 12, ext 2, second piece 32 + 1 L, end bonus 100, no z-drop):
//   packed 14 * 274 = 3836 <= 4000; U = 6, T = 4 + 28 = 32: 6 k < 32 up to k = 5, capped at 3; fourth: k = 4 > 3: no;
//   sixth: G = 14: 6 < 14 and 12 < 14, both below 100 + 4 and 28 + 4: bonus form 2.
#include <cstdio>
#include <cstring>

#include "../../hylight_amd/csrc/align_score_setup.h"

using namespace hlmi;

static hlmi_ava_opts long_opts() {
    hlmi_ava_opts o{};
    o.k = 19; o.w = 5; o.hpc = 1; o.min_chain_score = 100; o.max_gap = 10000; o.bandwidth = 2000; o.min_cnt = 3;
    o.min_mid_occ = 10; o.mid_occ_frac = 2e-4;
    o.match = 2; o.mismatch = 4; o.gap_open = 4; o.gap_ext = 2; o.ambi = 1;
    o.min_dp_score = 80; o.end_bonus = 0; o.pair_once = 1; o.gap_open2 = 24; o.gap_ext2 = 1; o.stub_oh = -1; o.zdrop = 400;
    return o;
}
static hlmi_ava_opts short_opts() {
    hlmi_ava_opts o{};
    o.k = 21; o.w = 11; o.hpc = 0; o.min_chain_score = 30; o.max_gap = 200; o.bandwidth = 50; o.min_cnt = 2;
    o.min_mid_occ = 1000; o.mid_occ_frac = 0.0;
    o.match = 4; o.mismatch = 2; o.gap_open = 12; o.gap_ext = 2; o.ambi = 1;
    o.min_dp_score = 60; o.end_bonus = 100; o.pair_once = 0; o.gap_open2 = 32; o.gap_ext2 = 1; o.stub_oh = -1; o.zdrop = 0;
    return o;
}

struct Want { int error, packed, bare, ext_all_long, go2, ge2, kmax, kgap1, kgap2, kshift, kext_plain, kext_bonus, trim_ok, one_ok; };
static int n_bad = 0;
static void expect(const char *name, const hlmi_ava_opts &o, const AlignScoreHooks &h, const Want &w) {
    const AlignScoreSetup s = align_score_setup(o, h);
    const Want got{(int)s.error, s.packed, s.bare, s.ext_all_long, s.go2, s.ge2, s.kmax, s.kgap1, s.kgap2, s.kshift, s.kext_plain,
                   s.kext_bonus, s.trim_ok, s.one_ok};
    if (memcmp(&got, &w, sizeof got) == 0) return;
    ++n_bad;
    const int *g = &got.error, *e = &w.error;
    printf("%s:", name);
    for (size_t k = 0; k < sizeof got / sizeof(int); ++k) printf(" %d%s", g[k], g[k] == e[k] ? "" : "(!)");
    printf("\n");
}

int main() {
    const AlignScoreHooks none;
    const hlmi_ava_opts L = long_opts(), S = short_opts();
    hlmi_ava_opts o;
    //                                  err pk bare all go2 ge2 kmax g1 g2 sh xp xb trim one
    expect("long", L, none,             {0, 1, 0, 0, 24, 1, 2, 1, 1, 1, 1, 0, 1, 1});
    expect("short", S, none,            {0, 1, 0, 0, 32, 1, 3, 1, 1, 0, 1, 2, 1, 1});
    // the other constants of tests/test_gpu_ava_structured.py
    o = L; o.gap_open2 = 0;
    expect("one_piece", o, none,        {0, 1, 0, 0, 0, 0, 2, 1, 1, 1, 1, 0, 1, 1});
    o = L; o.match = o.mismatch = o.gap_open = o.gap_ext = 1; o.gap_open2 = 0;
    expect("all_ones", o, none,         {0, 1, 0, 0, 0, 0, 2, 1, 1, 1, 1, 0, 1, 1});
    o = L; o.mismatch = 16; o.gap_open = 20; o.gap_ext = 2; o.gap_open2 = 0;      // 22 * 274 > 4000; a drop of 400 is 19 rows
    expect("wide_scores", o, none,      {0, 0, 0, 1, 0, 0, 2, 1, 0, 0, 1, 0, 1, 1});
    // z-drop: 378 is 63 rows down, 2 * 193 = 386 > 378; 390 is 65 rows, 382 is not > 390
    o = L; o.zdrop = 100;
    expect("zdrop 100", o, none,        {0, 1, 0, 1, 24, 1, 2, 1, 1, 1, 1, 0, 1, 1});
    o = L; o.zdrop = 378;
    expect("zdrop 378", o, none,        {0, 1, 0, 1, 24, 1, 2, 1, 1, 1, 1, 0, 1, 1});
    o = L; o.zdrop = 390;
    expect("zdrop 390", o, none,        {0, 1, 0, 0, 24, 1, 2, 1, 1, 1, 1, 0, 1, 1});
    o = L; o.match = 0;                 // no proof without a positive match score: every certificate off
    expect("match 0", o, none,          {0, 1, 0, 0, 24, 1, -1, 0, 0, 0, 0, 0, 1, 1});
    // stub rule: the candidates' tasks report scores only
    hlmi_ava_opts LS = L, SS = S;
    LS.stub_oh = 3; SS.stub_oh = 3;
    expect("long, stub rule", LS, none, {0, 1, 1, 0, 24, 1, 2, 1, 1, 1, 1, 0, 1, 1});
    expect("short, stub rule", SS, none, {0, 1, 1, 0, 32, 1, 3, 1, 1, 0, 1, 2, 1, 1});
    // every hook answer once
    AlignScoreHooks h;
    h = none; h.narrow_unpacked = true;
    expect("HLMI_NARROW_UNPACKED", LS, h,   {0, 0, 0, 0, 24, 1, 2, 1, 1, 1, 1, 0, 1, 1});
    h = none; h.stub_full_rows = true;
    expect("HLMI_STUB_FULL_ROWS", LS, h,    {0, 1, 0, 0, 24, 1, 2, 1, 1, 1, 1, 0, 1, 1});
    h = none; h.no_gap1_cert = true;        // (the seventh certificate builds on the fifth)
    expect("HLMI_NO_GAP1_CERT", LS, h,      {0, 1, 1, 0, 24, 1, 2, 0, 0, 1, 1, 0, 1, 1});
    h = none; h.no_gap2_cert = true;
    expect("HLMI_NO_GAP2_CERT", LS, h,      {0, 1, 1, 0, 24, 1, 2, 1, 0, 1, 1, 0, 1, 1});
    h = none; h.no_shift_cert = true;
    expect("HLMI_NO_SHIFT_CERT", LS, h,     {0, 1, 1, 0, 24, 1, 2, 1, 1, 0, 1, 0, 1, 1});
    h = none; h.no_ext_cert = true;
    expect("HLMI_NO_EXT_CERT", LS, h,       {0, 1, 1, 0, 24, 1, 2, 1, 1, 1, 0, 0, 1, 1});
    expect("HLMI_NO_EXT_CERT, short", S, h, {0, 1, 0, 0, 32, 1, 3, 1, 1, 0, 0, 0, 1, 1});
    h = none; h.no_one_piece_cert = true;
    expect("HLMI_NO_ONE_PIECE_CERT", LS, h, {0, 1, 1, 0, 24, 1, 2, 1, 1, 1, 1, 0, 1, 0});
    h = none; h.no_suffix_trim = true;
    expect("HLMI_NO_SUFFIX_TRIM", LS, h,    {0, 1, 1, 0, 24, 1, 2, 1, 1, 1, 1, 0, 0, 1});
    // the two refused option sets: a second piece that is the cheaper one at 15 bases (5 + 15 < 4 + 30), and tasks of more
    // than 32 000 rows (max_gap + 136; 31 864 is the last that fits)
    o = L; o.gap_open2 = 5; o.gap_ext2 = 1;
    expect("second piece too cheap", o, none, {ALIGN_SCORE_GAP2_CHEAP, 1, 0, 0, 5, 1, 2, 1, 0, 1, 1, 0, 1, 1});
    o = L; o.max_gap = 40000;
    expect("max_gap 40000", o, none,    {ALIGN_SCORE_ROWS, 1, 0, 0, 24, 1, 2, 1, 1, 1, 1, 0, 1, 1});
    o = L; o.max_gap = 31865;
    expect("max_gap 31865", o, none,    {ALIGN_SCORE_ROWS, 1, 0, 0, 24, 1, 2, 1, 1, 1, 1, 0, 1, 1});
    o = L; o.max_gap = 31864;
    expect("max_gap 31864", o, none,    {0, 1, 0, 0, 24, 1, 2, 1, 1, 1, 1, 0, 1, 1});
    if (n_bad) { printf("align_setup_host_check: %d rows differ (order: error packed bare ext_all_long go2 ge2 kmax kgap1 kgap2 kshift kext_plain kext_bonus trim_ok one_ok)\n", n_bad); return 1; }
    printf("align_setup_host_check: ok\n");
    return 0;
}
