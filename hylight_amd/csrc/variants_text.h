// variants_text.h - the host half of hlmi_variants / hlmi_variants_reads (include/hylight_mi.h) that is text and arithmetic: the
// record of every contig (those that never reached the device included), the alternative symbol of a site, site_rate, and the
// lines of the two files.  Host-only and free of any HIP include, as depth_text.h is: tests/capi/variants_host_check.cpp compiles
// it with the plain host compiler under the sanitizers.  The arithmetic is the header's: alt_frac = (double)v[alt] / (double)c,
// site_rate = (double)sites / (double)callable, one IEEE division each - compiled without contraction like the rest of the host
// code (there is no multiply-add to contract here, the flag is the build's).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <string_view>
#include <vector>

namespace hlmi {
namespace var {

constexpr int N_SYM = 5, S_DEL = 4;     // A C G T del, in the order of the tie rule

// A site as the device writes it: 24 bytes.  pos counts from the first covered contig's first position (cbase of the layout).
struct SiteRec {
    uint32_t pos;
    uint32_t v[N_SYM];
};

// what the device found, per covered contig ("slot": its place among the contigs with a selected row) and per site
struct DeviceVariants {
    std::vector<uint64_t> callable, ref_other, sites;       // per slot
    std::vector<SiteRec> recs;                              // ascending by pos
    uint64_t tiles = 0, tiles_revisited = 0;                // tiles of the layout, and those the second pass ran over
};

struct ContigVariants {
    std::string name;
    uint64_t length = 0, reads = 0, callable = 0, ref_other = 0, sites = 0;
};

struct VariantTotals {
    uint64_t contigs_covered = 0, positions = 0, callable = 0, ref_other = 0, sites = 0, sites_base = 0, sites_del = 0;
};

// 0..3 for A C G T of either case, -1 for any other byte
inline int own_symbol(unsigned char b) {
    b &= 0xdfu;
    return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1;
}

// the symbol other than `own` with the most votes, the first of A C G T del on a tie
inline int alt_symbol(const uint32_t v[N_SYM], int own) {
    int alt = -1;
    for (int k = 0; k < N_SYM; ++k)
        if (k != own && (alt < 0 || v[k] > v[alt])) alt = k;
    return alt;
}

// Every contig in file order.  rc: selected rows per contig; slot_of_contig: its slot when rc != 0.
inline std::vector<ContigVariants> contig_records(const std::vector<std::string> &names, const std::vector<uint64_t> &length,
                                                  const std::vector<uint32_t> &rc, const std::vector<uint32_t> &slot_of_contig,
                                                  const DeviceVariants &dev, VariantTotals *tot) {
    std::vector<ContigVariants> out(names.size());
    VariantTotals t;
    for (size_t c = 0; c < names.size(); ++c) {
        ContigVariants &r = out[c];
        r.name = names[c];
        r.length = length[c];
        r.reads = rc[c];
        if (rc[c]) {
            const uint32_t j = slot_of_contig[c];
            r.callable = dev.callable[j];
            r.ref_other = dev.ref_other[j];
            r.sites = dev.sites[j];
            ++t.contigs_covered;
        }
        t.positions += r.length;
        t.callable += r.callable;
        t.ref_other += r.ref_other;
        t.sites += r.sites;
    }
    if (tot) *tot = t;
    return out;
}

inline double site_rate(const ContigVariants &r) { return r.callable ? (double)r.sites / (double)r.callable : 0.0; }

// the lines of out_summary, without their '\n': the header line, then one per contig
inline std::vector<std::string> summary_lines(const std::vector<ContigVariants> &recs) {
    std::vector<std::string> lines;
    lines.reserve(recs.size() + 1);
    lines.push_back("#contig\tlength\treads\tcallable\tsites\tsite_rate");
    for (const ContigVariants &r : recs) {
        char buf[128];
        snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%llu\t%.6f", (unsigned long long)r.length, (unsigned long long)r.reads,
                 (unsigned long long)r.callable, (unsigned long long)r.sites, site_rate(r));
        lines.push_back(r.name + buf);
    }
    return lines;
}

// The lines of out_sites, without their '\n': the header line, then one per site - contigs in file order, positions ascending.
// seq: every contig's bytes as in the file; cbase: where every slot starts in the sites' positions, and the total behind the
// last.  Adds sites_base and sites_del to *tot.  A record outside its contig or on a byte that is not A C G T is no site of this
// call: -> false, and the caller refuses to write (the device and the host disagree).
inline bool site_lines(const std::vector<std::string> &names, const std::vector<std::string_view> &seq, const std::vector<uint32_t> &rc,
                       const std::vector<uint32_t> &slot_of_contig, const std::vector<uint32_t> &cbase, const DeviceVariants &dev,
                       std::vector<std::string> &lines, VariantTotals *tot) {
    lines.clear();
    lines.push_back("#contig\tpos\tref\tdepth\tA\tC\tG\tT\tdel\talt\talt_count\talt_frac");
    size_t k = 0;                               // next record
    const size_t n = dev.recs.size();
    for (size_t c = 0; c < names.size(); ++c) {
        if (!rc[c]) continue;
        const uint32_t j = slot_of_contig[c];
        const uint64_t b = cbase[j], e = cbase[j + 1];
        for (; k < n && dev.recs[k].pos < e; ++k) {
            const SiteRec &s = dev.recs[k];
            if (s.pos < b || s.pos - b >= seq[c].size()) return false;
            const unsigned char own_byte = (unsigned char)seq[c][s.pos - b];
            const int own = own_symbol(own_byte);
            if (own < 0) return false;
            const int alt = alt_symbol(s.v, own);
            uint64_t depth = 0;
            for (int q = 0; q < N_SYM; ++q) depth += s.v[q];
            if (!depth) return false;
            char buf[192];
            snprintf(buf, sizeof buf, "\t%llu\t%c\t%llu\t%u\t%u\t%u\t%u\t%u\t%c\t%u\t%.6f", (unsigned long long)(s.pos - b) + 1, "ACGT"[own],
                     (unsigned long long)depth, s.v[0], s.v[1], s.v[2], s.v[3], s.v[4], "ACGT*"[alt], s.v[alt],
                     (double)s.v[alt] / (double)depth);
            lines.push_back(names[c] + buf);
            if (tot) ++(alt == S_DEL ? tot->sites_del : tot->sites_base);
        }
    }
    return k == n;
}

}  // namespace var
}  // namespace hlmi
