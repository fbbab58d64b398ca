// Stand-alone check of the text arithmetic the kernels share with the host: hylight_amd/csrc/dec_text.h (decimal width, decimal
// digits, "%.4f" as an integer conversion), row_score.h (the three scores of a final row, the identity test, the sort key) and
// sr_overlaps.h (a PAF row as a SAVAGE overlap record and its line) - against printf, strtod and a restatement through text of
// the host code that came first (capi.cpp:hlmi_minimap22sfo, sfo.cpp).  Host compiler only, no GPU, no Python; the scores are
// IEEE doubles in a fixed evaluation order, so build without contraction, as the library is built:
//   g++ -std=c++17 -O1 -ffp-contract=off tests/capi/dec_text_host_check.cpp -o dec_text_host_check
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all ... (for the host sanitizers)
// Prints "dec_text_host_check: ok" and exits 0, or names the first mismatches of every part.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../hylight_amd/csrc/dec_text.h"
#include "../../hylight_amd/csrc/row_score.h"
#include "../../hylight_amd/csrc/sr_overlaps.h"

using namespace hlmi;

static long bad = 0;
static void mismatch(const char *part, const std::string &what) {
    if (++bad <= 20) printf("FAILED %s: %s\n", part, what.c_str());
}

// ---- dec_len / put_dec and the signed forms --------------------------------------------------------------------------------------
// the bytes in front of and behind the number stay as they were: a formatter writes its digits and nothing else
template <typename T, typename Len, typename Put>
static void check_number(const char *part, T v, const char *fmt, Len len, Put put) {
    char want[40], got[40];
    const int n = snprintf(want, sizeof want, fmt, v);
    memset(got, '#', sizeof got);
    char *end = put(got + 1, v);
    if (len(v) != n || end != got + 1 + n || memcmp(got + 1, want, (size_t)n) != 0 || got[0] != '#' || got[1 + n] != '#')
        mismatch(part, std::string("want ") + want + ", wrote " + std::string(got + 1, (size_t)(end > got + 1 && end < got + 39 ? end - got - 1 : 0)) +
                           ", length " + std::to_string(len(v)));
}
static void check_u32(uint32_t v) {
    check_number(
        "dec 32", v, "%" PRIu32, [](uint32_t x) { return dec_len(x); }, [](char *p, uint32_t x) { return put_dec(p, x); });
}
static void check_u64(uint64_t v) {
    check_number(
        "dec 64", v, "%" PRIu64, [](uint64_t x) { return dec_len(x); }, [](char *p, uint64_t x) { return put_dec(p, x); });
}
static void check_i32(int32_t v) {
    check_number(
        "signed 32", v, "%" PRId32, [](int32_t x) { return dec_len_signed(x); }, [](char *p, int32_t x) { return put_dec_signed(p, x); });
}
static void check_i64(int64_t v) {
    check_number(
        "signed 64", v, "%" PRId64, [](int64_t x) { return dec_len_signed(x); }, [](char *p, int64_t x) { return put_dec_signed(p, x); });
}
// a value of the unsigned set in every form that holds it: as it is, and negated
static void check_value(uint64_t v) {
    check_u64(v);
    if (v <= (uint64_t)INT64_MAX) { check_i64((int64_t)v); check_i64(-(int64_t)v); }
    if (v <= UINT32_MAX) check_u32((uint32_t)v);
    if (v <= (uint64_t)INT32_MAX) { check_i32((int32_t)v); check_i32(-(int32_t)v); }
}
static void check_decimal(std::mt19937_64 &rng) {
    check_value(0);
    uint64_t p = 1;
    for (int k = 0; k <= 19; ++k) {                          // 10^k - 1, 10^k, 10^k + 1 for every 10^k that fits
        check_value(p - 1); check_value(p); check_value(p + 1);
        if (k < 19) p *= 10;
    }
    check_value(UINT32_MAX); check_value((uint64_t)UINT32_MAX + 1);
    check_value(UINT64_MAX);
    check_value((uint64_t)INT32_MAX); check_value((uint64_t)INT64_MAX);
    check_i64(-1); check_i32(-1);
    check_i32(INT32_MIN); check_i64(INT64_MIN);              // the magnitude is an unsigned difference: in the domain
    for (int i = 0; i < 1000000; ++i) {                      // every width comes up: a random number of leading zero bits
        check_value(rng() >> (rng() % 64));                  // (10^6 values of at most 64 bits, and of them those of at most 32)
        check_u32((uint32_t)rng());
        check_i32((int32_t)(uint32_t)rng());
    }
}

// ---- "%.4f" ----------------------------------------------------------------------------------------------------------------------
static void check_fixed4(double v) {
    const bool in_range = !std::signbit(v) && std::isfinite(v) && v < 1099511627776.0;
    uint64_t q = 0;
    if (fixed4_q(v, q) != in_range) {
        char b[64];
        snprintf(b, sizeof b, "%a is %s the range", v, in_range ? "in" : "outside");
        return mismatch("fixed4 range", b);
    }
    if (!in_range) return;
    char want[64], got[64];
    const int n = snprintf(want, sizeof want, "%.4f", v);
    memset(got, '#', sizeof got);
    char *end = put_fixed4(got, q);
    if (fixed4_len(q) != n || end != got + n || memcmp(got, want, (size_t)n) != 0 || got[n] != '#') {
        char b[160];
        snprintf(b, sizeof b, "%a: want %s, length %d, wrote %.*s", v, want, fixed4_len(q), n, got);
        mismatch("fixed4", b);
    }
}
// the value classes of fixed4_check.cpp
static void check_fixed4_all(std::mt19937_64 &rng) {
    for (int j = 0; j <= 20; ++j)                             // the dyadic grid: every exact tie of the fourth decimal
        for (uint64_t k = 0; k < 4096; ++k) check_fixed4((double)k / (double)(1ull << j));
    for (int i = 0; i < 1000000; ++i) {                       // scores as the rows have them: ratios of small integers
        const double a = (double)(rng() % 100000), b = (double)(rng() % 100000 + 1);
        check_fixed4(a / b); check_fixed4(0.4 * (a / b) + 0.6 * (b / (a + b))); check_fixed4(1.0 - a / b);
    }
    for (int i = 0; i < 1000000; ++i) {                       // every exponent, random mantissas, both signs, specials
        uint64_t bits = rng();
        double v;
        memcpy(&v, &bits, 8);
        check_fixed4(v);
        check_fixed4(std::ldexp((double)(rng() >> 11), -(int)(rng() % 90)));
    }
    const double sp[] = {0.0, -0.0, 0.00005, 0.00015, 0.99995, 1.0, 0.5, 1e-300, 5e-324, 1099511627775.99995, 1099511627776.0, 1e14,
                         NAN, INFINITY, -INFINITY, -0.00004, -1.5};
    for (double v : sp) check_fixed4(v);
}

// ---- the scores of a row: filter_overlap_slr2.py:113,138-146 through printf and strtod --------------------------------------------
static void check_score(uint32_t nmatch, uint32_t blen, uint32_t qlen, uint32_t tlen, uint32_t xsum) {
    const double mc = (double)nmatch, ln = (double)blen;
    const double mlen = (double)((uint64_t)qlen + tlen) / 2.0;
    const double t1 = mc / mlen, t2 = mc / ln;
    const double a = 0.4 * t1, b = 0.6 * t2;
    const double score = a + b;
    const double mis = (double)xsum / mc;
    const double score2 = 1.0 - mis;
    char w1[64], w2[64], w3[64];
    snprintf(w1, sizeof w1, "%.4f", score);
    snprintf(w2, sizeof w2, "%.4f", score2);
    snprintf(w3, sizeof w3, "%.4f", t2);
    uint64_t key = 0;                                        // column 12 as sort_scored_lines reads it: its digits as one integer
    for (const char *p = w1; *p; ++p)
        if (*p != '.') key = key * 10 + (uint64_t)(*p - '0');
    const uint32_t want_key = key < SCORE_KEY_LIMIT ? (uint32_t)key : 0xffffffffu;
    char what[200];
    snprintf(what, sizeof what, "row %u %u %u %u x %u", nmatch, blen, qlen, tlen, xsum);
    for (const double iden : {0.95, 0.995}) {
        const int want = strtod(w2, nullptr) < iden ? SCORE_DROPPED : SCORE_KEPT;
        RowScore s;
        const int st = row_score(nmatch, blen, qlen, tlen, xsum, iden, s);
        if (st != want) { mismatch("score status", what); continue; }
        char g1[64], g2[64], g3[64];
        *put_fixed4(g1, s.q1) = 0; *put_fixed4(g2, s.q2) = 0; *put_fixed4(g3, s.q3) = 0;
        if (strcmp(g1, w1) || strcmp(g2, w2) || strcmp(g3, w3)) mismatch("score columns", std::string(what) + ": want " + w1 + " " + w2 + " " + w3 + ", got " + g1 + " " + g2 + " " + g3);
        if (s.key != want_key) mismatch("score key", what);
    }
}
static void check_scores(std::mt19937_64 &rng) {
    for (int i = 0; i < 1000000; ++i) {
        const uint32_t blen = 1 + (uint32_t)(rng() % 100000), nmatch = 1 + (uint32_t)(rng() % blen), xsum = (uint32_t)(rng() % (nmatch + 1));
        // reads of about the row's length, as rows have them, and now and then of any length (a score far from 1)
        const uint32_t spread = i % 4 ? blen / 8 + 2 : 200000;
        const uint32_t qlen = blen + (uint32_t)(rng() % spread), tlen = blen + (uint32_t)(rng() % spread);
        check_score(nmatch, blen, qlen, tlen, xsum);
        if (i % 10 == 0) {                                   // the edges: no X digit, nothing but X digits, a full match, an odd sum
            check_score(nmatch, blen, qlen, tlen, 0);
            check_score(nmatch, blen, qlen, tlen, nmatch);
            check_score(blen, blen, qlen, tlen, xsum % (blen + 1));
            check_score(nmatch, blen, qlen, tlen ^ ((qlen + tlen + 1) & 1u), xsum);
        }
    }
    // a row the exact conversion does not cover: no match (0 / 0), more X digits than matches (a negative score2)
    RowScore s;
    if (row_score(0, 0, 100, 100, 0, 0.95, s) != SCORE_GENERAL) mismatch("score status", "0 / 0 is not left to the general formatter");
    if (row_score(10, 20, 100, 100, 11, 0.95, s) != SCORE_GENERAL) mismatch("score status", "a negative score2 is not left to the general formatter");
}

// ---- sr_overlaps.h against the two host converters, restated over text -------------------------------------------------------------
struct PafRow {
    long long qname, tname;                                  // read names are numbers (sr_overlaps.hip: name_number)
    uint32_t qlen, qs, tlen, ts, te, nmatch, blen;
    bool rev;
};
// capi.cpp:hlmi_minimap22sfo -> the SFO row's eight fields
static std::vector<std::string> sfo_fields(const PafRow &r) {
    long long ql = r.qlen, qs = r.qs, tl = r.tlen, ts = r.ts, te = r.te, oha, ohb;
    if (!r.rev) { oha = qs - ts; ohb = tl - ts - (ql - qs); }
    else { oha = qs - (tl - te); ohb = te - (ql - qs); }
    const long long ola = oha >= 0 ? std::min(ql - oha, tl) : std::min(tl + oha, ql);
    std::string a = std::to_string(r.qname), b = std::to_string(r.tname);
    if (a > b) {                                             // ids in string order
        std::swap(a, b);
        if (!r.rev) { oha = -oha; ohb = -ohb; } else std::swap(oha, ohb);
    }
    return {a, b, r.rev ? "I" : "N", std::to_string(oha), std::to_string(ohb), std::to_string(ola), std::to_string(ola),
            std::to_string((long long)r.blen - (long long)r.nmatch)};
}
// sfo.cpp:42-51 -> the row of the sorted intermediate file, ten fields
static std::vector<std::string> sorted_fields(std::vector<std::string> f) {
    long long ia = atoll(f[0].c_str()), ib = atoll(f[1].c_str());
    if (ia > ib) {
        if (f[2] == "I") f = {f[1], f[0], f[2], f[4], f[3], f[6], f[5], f[7]};
        else f = {f[1], f[0], f[2], std::to_string(-atoll(f[3].c_str())), std::to_string(-atoll(f[4].c_str())), f[6], f[5], f[7]};
        std::swap(ia, ib);
    }
    f.insert(f.begin(), {std::to_string(ia), std::to_string(ib)});
    return f;
}
static std::string joined(const std::vector<std::string> &f) {
    std::string s;
    for (size_t i = 0; i < f.size(); ++i) { if (i) s += '\t'; s += f[i]; }
    return s;
}
// sfo.cpp:69-95 -> the 13-column line; empty: minlen <= 0
static std::string savage_line(const std::vector<std::string> &c) {
    const long long oha = atoll(c[5].c_str()), ohb = atoll(c[6].c_str()), ola = atoll(c[7].c_str()), olb = atoll(c[8].c_str());
    const char ori = c[4] == "N" ? '+' : '-';
    const long long ovlen = std::min(ola, olb);
    long long lena, lenb, pos1;
    std::string id1, id2;
    char ori1, ori2;
    if (oha >= 0) {
        lena = ola + oha + (ohb >= 0 ? 0 : -ohb);
        lenb = ohb >= 0 ? olb + ohb : olb;
        id1 = c[0]; id2 = c[1]; pos1 = oha; ori1 = '+'; ori2 = ori;
    } else {
        lena = ohb >= 0 ? ola : ola - ohb;
        lenb = -oha + olb + (ohb >= 0 ? ohb : 0);
        id1 = c[1]; id2 = c[0]; pos1 = -oha; ori1 = ori; ori2 = '+';
    }
    const long long minlen = std::min(lena, lenb);
    if (minlen <= 0) return std::string();
    const double x = (double)(100 * ovlen) / (double)minlen;
    long long perc = (long long)std::nearbyint(x);
    if (perc > 100) perc = 100;
    char buf[256];
    snprintf(buf, sizeof buf, "%s\t%s\t%lld\t-\t-\t%c\t%c\t%lld\t-\t%lld\t-\ts\ts", id1.c_str(), id2.c_str(), pos1, ori1, ori2, perc, ovlen);
    return buf;
}
static int sign(int c) { return c < 0 ? -1 : c > 0 ? 1 : 0; }

static void check_sr() {
    // the reads of the rows: ranks by number and by string disagree for 7 / 12 and agree for 10 / 11
    const long long names[4] = {7, 10, 11, 12};
    auto num_rank = [&](long long v) { uint32_t k = 0; for (long long w : names) k += w < v; return k; };
    auto str_rank = [&](long long v) { uint32_t k = 0; for (long long w : names) k += std::to_string(w) < std::to_string(v); return k; };
    // qlen qs tlen ts te: the query hangs out in front (oha > 0), the target does (oha < 0), both start together (oha == 0),
    // one read inside the other, and a row of equal reads end to end
    const uint32_t geo[][5] = {{1000, 400, 900, 0, 600},  {900, 0, 1000, 350, 900}, {800, 0, 800, 0, 800},   {500, 100, 2000, 700, 1100},
                               {2000, 650, 450, 0, 450},  {700, 20, 700, 20, 690},  {1200, 5, 1000, 0, 997}, {1000, 0, 1200, 203, 1200}};
    const long long ids[][2] = {{7, 12}, {12, 7}, {10, 11}, {11, 10}};
    struct Made { SrRec rec; std::string line; };
    std::vector<Made> made;
    int neg = 0, zero = 0, pos = 0;
    for (const auto &g : geo)
        for (const auto &id : ids)
            for (int rev = 0; rev < 2; ++rev) {
                const uint32_t blen = g[4] - g[3] + 7, nmatch = blen - (g[1] % 13);
                const PafRow r{id[0], id[1], g[0], g[1], g[2], g[3], g[4], nmatch, blen, rev != 0};
                const std::vector<std::string> want = sorted_fields(sfo_fields(r));
                SrRowIn in;
                in.qlen = r.qlen; in.qs = r.qs; in.tlen = r.tlen; in.ts = r.ts; in.te = r.te; in.nmatch = r.nmatch; in.blen = r.blen;
                in.rev = r.rev;
                in.q_str = str_rank(r.qname); in.t_str = str_rank(r.tname); in.q_num = num_rank(r.qname); in.t_num = num_rank(r.tname);
                const SrRec o = sr_record(in);
                const std::string a = std::to_string(names[o.na]), b = std::to_string(names[o.nb]);
                const std::string got = joined({a, b, a, b, o.rev ? "I" : "N", std::to_string(o.oha), std::to_string(o.ohb),
                                                std::to_string(o.ola), std::to_string(o.ola), std::to_string(o.k)});
                char what[120];
                snprintf(what, sizeof what, "row %lld %lld %c geometry %u %u %u %u %u", id[0], id[1], rev ? '-' : '+', g[0], g[1], g[2], g[3], g[4]);
                if (got != joined(want)) mismatch("sr_record", std::string(what) + ": want " + joined(want) + ", got " + got);
                (o.oha < 0 ? neg : o.oha == 0 ? zero : pos)++;
                // the line, written with the formatters the kernel writes it with
                const SrLine l = sr_line(o);
                const std::string want_line = savage_line(want);
                if ((l.minlen <= 0) != want_line.empty()) mismatch("sr_line", std::string(what) + ": minlen");
                else if (l.minlen > 0) {
                    char buf[256], *p = buf;
                    p = put_dec_signed(p, (int64_t)names[l.n1]); *p++ = '\t';
                    p = put_dec_signed(p, (int64_t)names[l.n2]); *p++ = '\t';
                    p = put_dec_signed(p, l.pos1);
                    p += sprintf(p, "\t-\t-\t%c\t%c\t", l.ori1, l.ori2);
                    p = put_dec_signed(p, l.perc);
                    p += sprintf(p, "\t-\t");
                    p = put_dec_signed(p, l.ovlen);
                    strcpy(p, "\t-\ts\ts");
                    if (want_line != buf) mismatch("sr_line", std::string(what) + ": want " + want_line + ", got " + buf);
                }
                made.push_back(Made{o, joined(want)});
            }
    if (!neg || !zero || !pos) mismatch("sr_record", "the rows do not reach oha < 0, == 0 and > 0");
    // the order of two rows of one id pair is the byte order of their lines (sfo.cpp:58-61)
    size_t compared = 0;
    for (const Made &x : made)
        for (const Made &y : made) {
            if (x.rec.na != y.rec.na || x.rec.nb != y.rec.nb) continue;
            ++compared;
            if (sign(sr_cmp_rec(x.rec, y.rec)) != sign(x.line.compare(y.line))) mismatch("sr_cmp_rec", x.line + " against " + y.line);
        }
    if (compared < 500) mismatch("sr_cmp_rec", "too few pairs of rows share an id pair");
}

int main() {
    std::mt19937_64 rng(20241019);
    check_decimal(rng);
    check_fixed4_all(rng);
    check_scores(rng);
    check_sr();
    if (bad) { printf("%ld checks failed\n", bad); return 1; }
    printf("dec_text_host_check: ok\n");
    return 0;
}
