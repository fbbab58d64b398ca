// variants_ins_text.h - the host half of hlmi_variants_ins / hlmi_variants_reads_ins (include/hylight_mi.h) that is text and
// arithmetic, beside variants_text.h: the insertion sites' records per contig, ins_rate, the lines of out_ins and the three columns
// the summary gains.  Host-only and free of any HIP include: tests/capi/variants_ins_host_check.cpp compiles it with the plain host
// compiler under the sanitizers.  The arithmetic is the header's: ins_frac = (double)(i + l) / (double)s, ins_rate =
// (double)ins_sites / (double)slots, one IEEE division each.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <string_view>
#include <vector>

#include "variants_text.h"

namespace hlmi {
namespace var {

constexpr uint32_t INS_CAP = 16;        // POLISH_INS_CAP of polish_internal.h (variants.hip asserts both)

// An insertion site as the device writes it: 40 bytes.  pos counts as SiteRec::pos does and is the slot's position p: the gap in
// front of position p of its contig.  The count pass's second run writes pos, span, ins and ins_long, the slot passes' last
// kernel len, len_count and seq (seq[j], j < len: A C G T or N; the bytes behind are not read).
struct InsRec {
    uint32_t pos;
    uint32_t span, ins, ins_long;       // s, i, l of the header
    uint32_t len, len_count;
    char seq[INS_CAP];
};

// what the device found about slots, per covered contig ("slot" of DeviceVariants) and per insertion site
struct DeviceInsertions {
    std::vector<uint64_t> slots_callable, ins_sites;        // per covered contig
    std::vector<InsRec> recs;                               // ascending by pos
    uint64_t slot_sites = 0;                                // sites with an inserting row: what the slot passes ran over
};

struct ContigInsertions {
    uint64_t slots = 0, ins_sites = 0;
};

struct InsTotals {
    uint64_t slots_callable = 0, ins_sites = 0;
};

// every contig in file order, as contig_records goes over them
inline std::vector<ContigInsertions> contig_insertions(const std::vector<uint32_t> &rc, const std::vector<uint32_t> &slot_of_contig,
                                                       const DeviceInsertions &dev, InsTotals *tot) {
    std::vector<ContigInsertions> out(rc.size());
    InsTotals t;
    for (size_t c = 0; c < rc.size(); ++c) {
        if (!rc[c]) continue;
        const uint32_t j = slot_of_contig[c];
        out[c].slots = dev.slots_callable[j];
        out[c].ins_sites = dev.ins_sites[j];
        t.slots_callable += out[c].slots;
        t.ins_sites += out[c].ins_sites;
    }
    if (tot) *tot = t;
    return out;
}

inline double ins_rate(const ContigInsertions &r) { return r.slots ? (double)r.ins_sites / (double)r.slots : 0.0; }

// the lines of out_summary of the _ins calls, without their '\n': summary_lines's, each with three columns more
inline std::vector<std::string> ins_summary_lines(const std::vector<ContigVariants> &recs, const std::vector<ContigInsertions> &ins) {
    std::vector<std::string> lines = summary_lines(recs);
    if (ins.size() != recs.size()) return {};               // (never: both are one entry per contig)
    lines[0] += "\tslots\tins_sites\tins_rate";
    for (size_t c = 0; c < ins.size(); ++c) {
        char buf[96];
        snprintf(buf, sizeof buf, "\t%llu\t%llu\t%.6f", (unsigned long long)ins[c].slots, (unsigned long long)ins[c].ins_sites,
                 ins_rate(ins[c]));
        lines[c + 1] += buf;
    }
    return lines;
}

// The lines of out_ins, without their '\n': the header line, then one per insertion site - contigs in file order, slots ascending.
// Arguments as site_lines takes them.  A record that does not fit its contig is no site of this call: pos outside 1..length-1,
// no spanning row, i + l > s, len_count > i, len > 16, a length without rows or rows without a length, a byte of seq that is
// none of A C G T N -> false, and the caller refuses to write (the device and the host disagree).
inline bool ins_lines(const std::vector<std::string> &names, const std::vector<std::string_view> &seq, const std::vector<uint32_t> &rc,
                      const std::vector<uint32_t> &slot_of_contig, const std::vector<uint32_t> &cbase, const DeviceInsertions &dev,
                      std::vector<std::string> &lines) {
    lines.clear();
    lines.push_back("#contig\tpos\tref\tspan\tins\tins_long\tins_frac\tlen\tlen_count\tseq");
    size_t k = 0;                               // next record
    const size_t n = dev.recs.size();
    for (size_t c = 0; c < names.size(); ++c) {
        if (!rc[c]) continue;
        const uint32_t j = slot_of_contig[c];
        const uint64_t b = cbase[j], e = cbase[j + 1];
        for (; k < n && dev.recs[k].pos < e; ++k) {
            const InsRec &s = dev.recs[k];
            if (s.pos <= b || s.pos - b >= seq[c].size()) return false;            // slot p: 0 < p < length
            const uint64_t p = s.pos - b, alt = (uint64_t)s.ins + s.ins_long;
            if (!s.span || alt > s.span || s.len_count > s.ins || s.len > INS_CAP) return false;
            if ((s.len == 0) != (s.ins == 0) || (s.len == 0) != (s.len_count == 0)) return false;
            std::string bases(s.seq, s.len);
            for (const char ch : bases)
                if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T' && ch != 'N') return false;
            if (bases.empty()) bases = "*";
            unsigned char ref = (unsigned char)seq[c][p - 1];
            if (ref >= 'a' && ref <= 'z') ref &= 0xdfu;
            char buf[192];
            snprintf(buf, sizeof buf, "\t%llu\t%c\t%u\t%u\t%u\t%.6f\t%u\t%u\t", (unsigned long long)p, (char)ref, s.span, s.ins, s.ins_long,
                     (double)alt / (double)s.span, s.len, s.len_count);
            lines.push_back(names[c] + buf + bases);
        }
    }
    return k == n;
}

}  // namespace var
}  // namespace hlmi
