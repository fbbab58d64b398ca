// phase_text.h - the host half of hlmi_phase / hlmi_phase_reads (include/hylight_mi.h) that is text and arithmetic: the sites with
// their own and alternative symbols from hlmi_variants's records, the link rule, the blocks and phase bits, the hap rule and the
// lines of the three files.  Host-only and free of any HIP include, as variants_text.h is: tests/capi/phase_host_check.cpp compiles
// it with the plain host compiler under the sanitizers.  The arithmetic is the header's: agree = (double)top / (double)inf, one
// IEEE division - compiled without contraction like the rest of the host code (there is no multiply-add to contract here, the
// flag is the build's).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <string_view>
#include <vector>

#include "variants_text.h"

namespace hlmi {
namespace ph {

// A site of hlmi_variants with what the phasing needs of it.  gpos counts as SiteRec::pos does, pos inside the contig (0-based).
struct PSite {
    uint32_t contig, pos, gpos;
    int own, alt;                       // 0..3 = A C G T; alt may be var::S_DEL
    uint32_t v[var::N_SYM];
};
// the four counters of the link between two consecutive sites as the device writes them: 16 bytes; the first digit is the
// allele at the left site
struct LinkCounts {
    uint32_t n00, n01, n10, n11;
};
// what the device writes per (row, block): 24 bytes.  block: the block's index among all blocks of the call, ascending
struct ReadRec {
    uint32_t row, block, spanned, a, b, other;
};
// an allele byte of the device's table
enum : uint8_t { AL_OWN = 0, AL_ALT = 1, AL_OTHER = 2, AL_NONE = 0xff };

enum : uint8_t { LINK_UNPHASED = 0, LINK_CIS = 1, LINK_TRANS = 2, LINK_ABSENT = 0xff };     // ABSENT: the two sites lie on two contigs
struct LinkCall {
    uint64_t inf = 0, top = 0;
    double agree = 0.0;
    uint8_t phased = LINK_UNPHASED;
};
// rule 3: phased iff inf >= min_link and (double)top / (double)inf >= min_agree (min_link >= 1: a phased link has inf >= 1)
inline LinkCall link_call(const LinkCounts &c, int min_link, double min_agree) {
    LinkCall r;
    const uint64_t cis = (uint64_t)c.n00 + c.n11, trans = (uint64_t)c.n01 + c.n10;
    r.inf = cis + trans;
    r.top = cis > trans ? cis : trans;
    if (r.inf) r.agree = (double)r.top / (double)r.inf;
    if (r.inf && r.inf >= (uint64_t)min_link && r.agree >= min_agree) r.phased = cis > trans ? LINK_CIS : LINK_TRANS;
    return r;
}

// The sites of every covered contig in file order, ascending, from hlmi_variants's records (variants_text.h: site_lines reads
// them the same way).  A record outside its contig, on a byte that is not A C G T or without a vote is no site: -> false.
inline bool phase_sites(const std::vector<std::string_view> &seq, const std::vector<uint32_t> &rc, const std::vector<uint32_t> &slot_of_contig,
                        const std::vector<uint32_t> &cbase, const var::DeviceVariants &dev, std::vector<PSite> &out) {
    out.clear();
    size_t k = 0;
    const size_t n = dev.recs.size();
    for (size_t c = 0; c < seq.size(); ++c) {
        if (!rc[c]) continue;
        const uint32_t j = slot_of_contig[c];
        const uint64_t b = cbase[j], e = cbase[j + 1];
        for (; k < n && dev.recs[k].pos < e; ++k) {
            const var::SiteRec &s = dev.recs[k];
            if (s.pos < b || s.pos - b >= seq[c].size()) return false;
            if (!out.empty() && out.back().gpos >= s.pos) return false;
            PSite p;
            p.contig = (uint32_t)c;
            p.pos = (uint32_t)(s.pos - b);
            p.gpos = s.pos;
            p.own = var::own_symbol((unsigned char)seq[c][p.pos]);
            if (p.own < 0) return false;
            p.alt = var::alt_symbol(s.v, p.own);
            uint64_t depth = 0;
            for (int q = 0; q < var::N_SYM; ++q) { p.v[q] = s.v[q]; depth += s.v[q]; }
            if (!depth) return false;
            out.push_back(p);
        }
    }
    return k == n;
}

// rule 4.  call: one byte per pair of neighbouring sites (sites.size() - 1 of them); index: the site's block among all blocks,
// ascending; first: every block's first site
struct Blocks {
    std::vector<uint8_t> call, bit;
    std::vector<uint32_t> index, first;
    uint64_t links = 0, links_phased = 0, blocks_multi = 0, sites_phased = 0;
};
// links: the counters of every pair of neighbouring sites (those across a contig junction are not read)
inline Blocks build_blocks(const std::vector<PSite> &sites, const std::vector<LinkCounts> &links, int min_link, double min_agree) {
    Blocks B;
    const size_t n = sites.size();
    B.bit.assign(n, 0);
    B.index.assign(n, 0);
    B.call.assign(n ? n - 1 : 0, LINK_ABSENT);
    size_t len = 0;                             // sites of the block being built
    auto close = [&]() {
        if (len >= 2) { ++B.blocks_multi; B.sites_phased += len; }
    };
    for (size_t i = 0; i < n; ++i) {
        uint8_t c = LINK_ABSENT;
        if (i && sites[i - 1].contig == sites[i].contig) {
            c = i - 1 < links.size() ? link_call(links[i - 1], min_link, min_agree).phased : (uint8_t)LINK_UNPHASED;
            ++B.links;
            B.links_phased += c == LINK_CIS || c == LINK_TRANS;
        }
        if (i) B.call[i - 1] = c;
        if (c == LINK_CIS || c == LINK_TRANS) {
            B.bit[i] = B.bit[i - 1] ^ (uint8_t)(c == LINK_TRANS);
            ++len;
        } else {
            close();
            B.first.push_back((uint32_t)i);
            len = 1;
        }
        B.index[i] = (uint32_t)B.first.size() - 1;
    }
    close();
    return B;
}

// rule 5
inline char hap_of(uint32_t a, uint32_t b) { return a > b ? 'A' : b > a ? 'B' : '-'; }

// one line of out_sites; first: the first site of the site's block, phase: the text of the last column
inline std::string phase_site_line(const std::vector<std::string> &names, const PSite &s, const PSite &first, const char *phase) {
    uint64_t depth = 0;
    for (int q = 0; q < var::N_SYM; ++q) depth += s.v[q];
    char buf[160];
    snprintf(buf, sizeof buf, "\t%llu\t%c\t%c\t%llu\t%u\t%u\t%llu\t%s", (unsigned long long)s.pos + 1, "ACGT"[s.own], "ACGT*"[s.alt],
             (unsigned long long)depth, s.v[s.own], s.v[s.alt], (unsigned long long)first.pos + 1, phase);
    return names[s.contig] + buf;
}

inline std::vector<std::string> phase_site_lines(const std::vector<std::string> &names, const std::vector<PSite> &sites, const Blocks &B) {
    std::vector<std::string> lines;
    lines.reserve(sites.size() + 1);
    lines.push_back("#contig\tpos\tref\talt\tdepth\tref_count\talt_count\tblock\tphase");
    for (size_t i = 0; i < sites.size(); ++i) lines.push_back(phase_site_line(names, sites[i], sites[B.first[B.index[i]]], B.bit[i] ? "1|0" : "0|1"));
    return lines;
}

// one line of out_links: the link between the sites a and b (a in front of b, one contig) with the counters c
inline std::string phase_link_line(const std::vector<std::string> &names, const PSite &a, const PSite &b, const LinkCounts &c, int min_link,
                                   double min_agree) {
    const LinkCall k = link_call(c, min_link, min_agree);
    char buf[192];
    snprintf(buf, sizeof buf, "\t%llu\t%llu\t%u\t%u\t%u\t%u\t%llu\t%.6f\t%s", (unsigned long long)a.pos + 1, (unsigned long long)b.pos + 1, c.n00,
             c.n01, c.n10, c.n11, (unsigned long long)k.inf, k.agree, k.phased == LINK_CIS ? "cis" : k.phased == LINK_TRANS ? "trans" : "-");
    return names[a.contig] + buf;
}

inline std::vector<std::string> phase_link_lines(const std::vector<std::string> &names, const std::vector<PSite> &sites,
                                                 const std::vector<LinkCounts> &links, int min_link, double min_agree) {
    std::vector<std::string> lines;
    lines.push_back("#contig\tpos1\tpos2\tn00\tn01\tn10\tn11\tinformative\tagree\tphased");
    for (size_t i = 0; i + 1 < sites.size() && i < links.size(); ++i) {
        if (sites[i].contig != sites[i + 1].contig) continue;
        lines.push_back(phase_link_line(names, sites[i], sites[i + 1], links[i], min_link, min_agree));
    }
    return lines;
}

struct ReadTotals {
    uint64_t records = 0, a = 0, b = 0, tie = 0;
};
// The records of rule 5 in the device's order (rows in selection order, a row's blocks ascending); those with nothing to say are
// dropped here.  read_of_row: the read record of every selected row - may be empty when lines == nullptr (the totals alone).
// A record that names a block or a row that does not exist: -> false.
inline bool phase_read_lines(const std::vector<std::string> &contig_names, const std::vector<std::string> &read_names,
                             const std::vector<uint32_t> &read_of_row, const std::vector<PSite> &sites, const Blocks &B,
                             const std::vector<ReadRec> &recs, std::vector<std::string> *lines, ReadTotals *tot) {
    if (lines) {
        lines->clear();
        lines->push_back("#read\tcontig\tblock\tspanned\thap_a\thap_b\tother\thap");
    }
    ReadTotals t;
    for (const ReadRec &r : recs) {
        if (r.block >= B.first.size()) return false;
        if ((uint64_t)r.a + r.b + r.other < 1) continue;
        const char h = hap_of(r.a, r.b);
        ++t.records;
        ++(h == 'A' ? t.a : h == 'B' ? t.b : t.tie);
        if (!lines) continue;
        if (r.row >= read_of_row.size() || read_of_row[r.row] >= read_names.size()) return false;
        const PSite &s = sites[B.first[r.block]];
        char buf[128];
        snprintf(buf, sizeof buf, "\t%llu\t%u\t%u\t%u\t%u\t%c", (unsigned long long)s.pos + 1, r.spanned, r.a, r.b, r.other, h);
        lines->push_back(read_names[read_of_row[r.row]] + "\t" + contig_names[s.contig] + buf);
    }
    if (tot) *tot = t;
    return true;
}

}  // namespace ph
}  // namespace hlmi
