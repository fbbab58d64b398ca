// dec_text.h - numbers as decimal text, the one definition for the kernels that write text (row_text.hip, sr_overlaps.hip,
// vq_next.hip, vq_merge.hip) and for paf_io.cpp: the bytes a number takes, the bytes, and "%.4f" as an exact integer conversion.
// tests/capi/dec_text_host_check.cpp compiles this file with the host compiler alone and compares every function with printf.
// 32- and 64-bit forms are separate on purpose: a 64-bit division is a long sequence on the device, and the vq kernels never
// need one.  Every loop has an explicit bound: a uint32_t has at most 9 digits behind its first, a uint64_t 19.
#pragma once
#include <cstdint>

#include "hd.h"

namespace hlmi {
// ---- unsigned: bytes of "%u" / "%llu", and the bytes themselves (-> behind the last digit) ---------------------------------------
HLMI_HD int dec_len(uint32_t v) {
    int n = 1;
    for (int k = 0; k < 9 && v >= 10; ++k) { v /= 10; ++n; }
    return n;
}
HLMI_HD int dec_len(uint64_t v) {
    int n = 1;
    for (int k = 0; k < 19 && v >= 10; ++k) { v /= 10; ++n; }
    return n;
}
HLMI_HD char *put_dec(char *p, uint32_t v) {
    const int n = dec_len(v);                                // <= 10
    for (int i = n - 1; i >= 0; --i) { p[i] = (char)('0' + v % 10); v /= 10; }
    return p + n;
}
HLMI_HD char *put_dec(char *p, uint64_t v) {
    const int n = dec_len(v);                                // <= 20
    for (int i = n - 1; i >= 0; --i) { p[i] = (char)('0' + (int)(v % 10)); v /= 10; }
    return p + n;
}
// ---- signed: "%d" / "%lld".  Every value of the type, the smallest included: the magnitude is taken as an unsigned difference ----
HLMI_HD int dec_len_signed(int32_t v) { return v < 0 ? 1 + dec_len(0u - (uint32_t)v) : dec_len((uint32_t)v); }
HLMI_HD int dec_len_signed(int64_t v) { return v < 0 ? 1 + dec_len((uint64_t)0 - (uint64_t)v) : dec_len((uint64_t)v); }
HLMI_HD char *put_dec_signed(char *p, int32_t v) {
    if (v < 0) { *p++ = '-'; return put_dec(p, 0u - (uint32_t)v); }
    return put_dec(p, (uint32_t)v);
}
HLMI_HD char *put_dec_signed(char *p, int64_t v) {
    if (v < 0) { *p++ = '-'; return put_dec(p, (uint64_t)0 - (uint64_t)v); }
    return put_dec(p, (uint64_t)v);
}
// ---- "%.4f" of a finite v in [0, 2^40): q = v x 10^4 rounded to nearest, ties to even - the rounding glibc's printf applies to
// the exact binary value in the default rounding mode.  v = m x 2^e, so v x 10^4 = (m x 10^4) >> -e.  false: v is not in that
// range (negative, -0.0 included; non-finite; >= 2^40) and q is not written: the caller takes a general formatter.
HLMI_HD bool fixed4_q(double v, uint64_t &q) {
    uint64_t bits;
    __builtin_memcpy(&bits, &v, 8);
    const int be = (int)((bits >> 52) & 0x7ff);
    if ((bits >> 63) || be == 0x7ff || !(v < 1099511627776.0)) return false;
    uint64_t m = bits & ((1ull << 52) - 1);
    int e = be - 1075;                                       // v = m x 2^e
    if (be) m |= 1ull << 52; else e = -1074;
    if (e >= 0) { q = (m << e) * 10000ull; return true; }    // (an integer below 2^40)
    const unsigned __int128 N = (unsigned __int128)m * 10000u;        // < 2^67
    const int sh = -e;
    if (sh > 68) { q = 0; return true; }                     // below a half: rounds to zero
    q = (uint64_t)(N >> sh);
    const unsigned __int128 rem = N & (((unsigned __int128)1 << sh) - 1), half = (unsigned __int128)1 << (sh - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    return true;
}
HLMI_HD int fixed4_len(uint64_t q) { return dec_len(q / 10000u) + 5; }
HLMI_HD char *put_fixed4(char *p, uint64_t q) {
    p = put_dec(p, q / 10000u);
    uint32_t fp = (uint32_t)(q % 10000u);
    *p++ = '.';
    p[3] = (char)('0' + fp % 10); fp /= 10;
    p[2] = (char)('0' + fp % 10); fp /= 10;
    p[1] = (char)('0' + fp % 10); fp /= 10;
    p[0] = (char)('0' + fp);
    return p + 4;
}
}  // namespace hlmi
