// sr_overlaps.h - one kept PAF row as a SAVAGE overlap record: the arithmetic of minimap22sfo.py (capi.cpp:200-216) and of
// sfo2overlaps.py --num_pairs 0 (sfo.cpp:43-95) on integers, shared by the kernels of sr_overlaps.hip and by the host check
// tests/capi/dec_text_host_check.cpp (which compiles this file with a host compiler only).
#pragma once
#include <cstdint>

#include "dec_text.h"

namespace hlmi {

// The row of sfo2overlaps' sorted intermediate file, "ida idb ida idb O oha ohb ola olb k": the smaller NUMBER first.  The ids
// are kept as numeric ranks (na < nb orders like the numbers do); olb == ola on this path.
struct SrRec {
    int64_t oha, ohb, ola;
    uint32_t na, nb;          // numeric rank of ida / idb among the reads of the call
    uint32_t k;               // column 11 - column 10 of the PAF row (the SFO row's last field; it only orders lines)
    uint32_t rev;             // 1: 'I', 0: 'N'
};

// what one PAF row carries into the record: q / t name ranks in STRING order and in NUMERIC order
struct SrRowIn {
    uint32_t qlen, qs, tlen, ts, te, nmatch, blen;
    uint32_t rev;
    uint32_t q_str, t_str, q_num, t_num;
};

HLMI_HD SrRec sr_record(const SrRowIn &r) {
    const int64_t ql = r.qlen, qs = r.qs, tl = r.tlen, ts = r.ts, te = r.te;
    int64_t oha, ohb;
    if (!r.rev) { oha = qs - ts; ohb = tl - ts - (ql - qs); }                 // minimap22sfo.py:45-60 (capi.cpp:205-206)
    else { oha = qs - (tl - te); ohb = te - (ql - qs); }
    const int64_t ola = oha >= 0 ? (ql - oha < tl ? ql - oha : tl) : (tl + oha < ql ? tl + oha : ql);
    uint32_t na = r.q_num, nb = r.t_num;
    if (r.q_str > r.t_str) {                                                   // ids in STRING order (capi.cpp:209-212)
        const uint32_t t = na; na = nb; nb = t;
        if (!r.rev) { oha = -oha; ohb = -ohb; } else { const int64_t t2 = oha; oha = ohb; ohb = t2; }
    }
    if (na > nb) {                                                             // the smaller NUMBER first (sfo.cpp:43-48)
        const uint32_t t = na; na = nb; nb = t;
        if (r.rev) { const int64_t t2 = oha; oha = ohb; ohb = t2; } else { oha = -oha; ohb = -ohb; }
    }
    SrRec o;
    o.oha = oha; o.ohb = ohb; o.ola = ola; o.na = na; o.nb = nb; o.k = r.blen - r.nmatch; o.rev = r.rev;
    return o;
}

// ---- the byte order of two decimal texts that are followed by the same byte below '-' and the digits (TAB, or the end of
// the line): '-' sorts below the digits, and of two digit strings where one is a prefix of the other the shorter is smaller
HLMI_HD int sr_cmp_digits(uint64_t a, uint64_t b) {        // a, b < 10^18
    const int la = dec_len(a), lb = dec_len(b);
    uint64_t x = a, y = b;
    for (int i = la; i < lb; ++i) x *= 10;                  // left-aligned: the shorter one padded with zeros
    for (int i = lb; i < la; ++i) y *= 10;
    if (x != y) return x < y ? -1 : 1;
    return la == lb ? 0 : (la < lb ? -1 : 1);
}
HLMI_HD int sr_cmp_dec_text(int64_t a, int64_t b) {
    if ((a < 0) != (b < 0)) return a < 0 ? -1 : 1;
    return sr_cmp_digits((uint64_t)(a < 0 ? -a : a), (uint64_t)(b < 0 ? -b : b));
}
// whole-line order of two rows of one id pair (sfo.cpp:58-61: the four numeric keys are equal, the line decides)
HLMI_HD int sr_cmp_rec(const SrRec &a, const SrRec &b) {
    if (a.rev != b.rev) return a.rev ? -1 : 1;              // 'I' < 'N'
    int c = sr_cmp_dec_text(a.oha, b.oha);
    if (c) return c;
    c = sr_cmp_dec_text(a.ohb, b.ohb);
    if (c) return c;
    c = sr_cmp_dec_text(a.ola, b.ola);                      // (twice in the line: ola and olb)
    if (c) return c;
    return sr_cmp_digits(a.k, b.k);
}

// The 13-column line of a record (sfo.cpp:70-94), ids still as numeric ranks.  minlen <= 0 is the caller's to refuse.
struct SrLine {
    uint32_t n1, n2;          // numeric ranks of the line's first and second id
    int64_t pos1, perc, ovlen, minlen;
    char ori1, ori2;
};
HLMI_HD SrLine sr_line(const SrRec &c) {
    const char ori = c.rev ? '-' : '+';
    const int64_t oha = c.oha, ohb = c.ohb, ola = c.ola, olb = c.ola;
    int64_t lena, lenb;
    SrLine l;
    l.ovlen = ola < olb ? ola : olb;
    if (oha >= 0) {
        lena = ola + oha + (ohb >= 0 ? 0 : -ohb);
        lenb = ohb >= 0 ? olb + ohb : olb;
        l.n1 = c.na; l.n2 = c.nb; l.pos1 = oha; l.ori1 = '+'; l.ori2 = ori;
    } else {
        lena = ohb >= 0 ? ola : ola - ohb;
        lenb = -oha + olb + (ohb >= 0 ? ohb : 0);
        l.n1 = c.nb; l.n2 = c.na; l.pos1 = -oha; l.ori1 = ori; l.ori2 = '+';
    }
    l.minlen = lena < lenb ? lena : lenb;
    l.perc = 0;
    if (l.minlen > 0) {
        // Python round(): half to even on the double 100 * ovlen / minlen (the division is correctly rounded on both sides)
        const double x = (double)(100 * l.ovlen) / (double)l.minlen;
        l.perc = (int64_t)__builtin_rint(x);
        if (l.perc > 100) l.perc = 100;
    }
    return l;
}
HLMI_HD bool sr_line_equal(const SrLine &a, const SrLine &b) {
    return a.n1 == b.n1 && a.n2 == b.n2 && a.pos1 == b.pos1 && a.perc == b.perc && a.ovlen == b.ovlen && a.ori1 == b.ori1 &&
           a.ori2 == b.ori2;
}

}  // namespace hlmi
