// phase_ins_text.h - the host half of hlmi_phase_ins / hlmi_phase_reads_ins (include/hylight_mi.h) that is text and arithmetic: which
// insertion sites of hlmi_variants_ins take part, the merge of the position sites and the insertion sites into one ascending list
// (slot p directly in front of position p), the site, link and read lines with their `+` marks and the three counters the stats
// gain.  The link rule, the block rule, the hap rule and the lines' formats are phase_text.h's and phase_reach_text.h's, called
// and not restated.  Host-only and free of any HIP include, as they are: tests/capi/phase_ins_host_check.cpp compiles it with the
// plain host compiler under the sanitizers.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <string_view>
#include <vector>

#include "phase_reach_text.h"
#include "phase_text.h"
#include "variants_ins_text.h"

namespace hlmi {
namespace ph {

// An insertion site takes part iff its called length has the support a position site's alt needs
inline bool ins_takes_part(const var::InsRec &r, int min_alt) { return r.len >= 1 && min_alt >= 0 && r.len_count >= (uint32_t)min_alt; }

// the order of the merged list in the device's position space (g < 2^31: polish_layout refuses more, so the key fits 32 bits):
// slot g sorts directly in front of position g
inline uint32_t site_key(uint32_t g, bool slot) { return 2u * g + (slot ? 0u : 1u); }

// The merged list.  sites[i] is what the link and block code reads (contig) and what the lines print: at an insertion site at
// slot p, pos = p - 1 - the anchor base, whose 1-based position p the files print - and own, alt and v are not read.
// ins_of[i]: the site's record in `ins`, -1 at a position site.
struct MergedSites {
    std::vector<PSite> sites;
    std::vector<uint32_t> key;                  // site_key, ascending strictly
    std::vector<int32_t> ins_of;
    std::vector<var::InsRec> ins;               // the insertion sites that take part, ascending
    std::vector<char> anchor;                   // per entry of ins: the upper-cased contig byte in front of the slot
    uint64_t ins_sites_phasing = 0, ins_sites_left_out = 0;
    bool slot(size_t i) const { return ins_of[i] >= 0; }
};

// positions: phase_sites's output; dev: hlmi_variants_ins's records over the same rows.  Arguments as phase_sites takes them.
// An insertion record outside 1 .. length - 1 of its contig or of more than 16 bases -> false (ins_lines refuses the same).
inline bool merge_sites(const std::vector<std::string_view> &seq, const std::vector<uint32_t> &rc, const std::vector<uint32_t> &slot_of_contig,
                        const std::vector<uint32_t> &cbase, const std::vector<PSite> &positions, const var::DeviceInsertions &dev, int min_alt,
                        MergedSites &out) {
    out = MergedSites{};
    size_t a = 0, k = 0;                        // next position site, next insertion record
    const size_t na = positions.size(), nk = dev.recs.size();
    for (size_t c = 0; c < seq.size(); ++c) {
        if (!rc[c]) continue;
        const uint32_t j = slot_of_contig[c];
        const uint64_t b = cbase[j], e = cbase[j + 1];
        for (;;) {
            for (; k < nk && dev.recs[k].pos < e && !ins_takes_part(dev.recs[k], min_alt); ++k) {
                if (dev.recs[k].pos <= b) return false;
                ++out.ins_sites_left_out;
            }
            const bool has_a = a < na && positions[a].gpos < e, has_k = k < nk && dev.recs[k].pos < e;
            if (!has_a && !has_k) break;
            if (has_a && positions[a].contig != c) return false;
            const bool slot = has_k && (!has_a || site_key(dev.recs[k].pos, true) < site_key(positions[a].gpos, false));
            if (!slot) {
                out.sites.push_back(positions[a]);
                out.key.push_back(site_key(positions[a].gpos, false));
                out.ins_of.push_back(-1);
                ++a;
            } else {
                const var::InsRec &r = dev.recs[k];
                if (r.pos <= b || r.pos - b >= seq[c].size() || r.len > var::INS_CAP) return false;
                PSite s{};
                s.contig = (uint32_t)c;
                s.pos = (uint32_t)(r.pos - b) - 1;
                s.gpos = r.pos;
                out.sites.push_back(s);
                out.key.push_back(site_key(r.pos, true));
                out.ins_of.push_back((int32_t)out.ins.size());
                out.ins.push_back(r);
                unsigned char ref = (unsigned char)seq[c][s.pos];
                if (ref >= 'a' && ref <= 'z') ref &= 0xdfu;
                out.anchor.push_back((char)ref);
                ++out.ins_sites_phasing;
                ++k;
            }
            const size_t n = out.key.size();
            if (n >= 2 && out.key[n - 2] >= out.key[n - 1]) return false;
        }
    }
    return a == na && k == nk;
}

// insertion sites that are members (not bridged) of a block of two or more members
inline uint64_t ins_sites_phased(const MergedSites &M, const Blocks &B) {
    std::vector<uint32_t> members(B.first.size(), 0);
    for (size_t i = 0; i < M.sites.size(); ++i) members[B.index[i]] += B.bit[i] != BIT_BRIDGED;
    uint64_t n = 0;
    for (size_t i = 0; i < M.sites.size(); ++i) n += M.slot(i) && B.bit[i] != BIT_BRIDGED && members[B.index[i]] >= 2;
    return n;
}

// `+` behind field `field` (0-based, tab-separated) of a line
inline void mark_field(std::string &line, int field) {
    size_t at = 0;                              // where the field starts, then where it ends
    for (int f = 0; f < field && at != std::string::npos; ++f) {
        at = line.find('\t', at);
        if (at != std::string::npos) ++at;
    }
    if (at != std::string::npos) at = line.find('\t', at);
    line.insert(at == std::string::npos ? line.size() : at, 1, '+');
}

inline const char *phase_text_of(uint8_t bit) { return bit == BIT_BRIDGED ? "." : bit ? "1|0" : "0|1"; }

// out_sites: a position site's line is phase_site_line's; an insertion site prints pos = p, the anchor base, `+` and the called
// bases, span, span - ins - ins_long, len_count.  A block whose first site is an insertion site has `+` behind its id.
inline std::vector<std::string> phase_ins_site_lines(const std::vector<std::string> &names, const MergedSites &M, const Blocks &B) {
    std::vector<std::string> lines;
    lines.reserve(M.sites.size() + 1);
    lines.push_back("#contig\tpos\tref\talt\tdepth\tref_count\talt_count\tblock\tphase");
    for (size_t i = 0; i < M.sites.size(); ++i) {
        const size_t f = B.first[B.index[i]];
        const PSite &s = M.sites[i], &first = M.sites[f];
        std::string line;
        if (!M.slot(i)) {
            line = phase_site_line(names, s, first, phase_text_of(B.bit[i]));
        } else {
            const var::InsRec &r = M.ins[(size_t)M.ins_of[i]];
            char buf[160];
            snprintf(buf, sizeof buf, "\t%llu\t%c\t+%.*s\t%u\t%u\t%u\t%llu\t%s", (unsigned long long)s.pos + 1, M.anchor[(size_t)M.ins_of[i]],
                     (int)r.len, r.seq, r.span, r.span - r.ins - r.ins_long, r.len_count, (unsigned long long)first.pos + 1, phase_text_of(B.bit[i]));
            line = names[s.contig] + buf;
        }
        if (M.slot(f)) mark_field(line, 7);
        lines.push_back(line);
    }
    return lines;
}

// out_links: phase_reach_link_lines's lines; a slot endpoint carries a trailing `+`
inline std::vector<std::string> phase_ins_link_lines(const std::vector<std::string> &names, const MergedSites &M, const ReachLinks &L, int min_link,
                                                     double min_agree) {
    std::vector<std::string> lines = phase_reach_link_lines(names, M.sites, L, min_link, min_agree);
    size_t k = 1;
    for (size_t i = 0; i + 1 < M.sites.size(); ++i)
        for (int d = 1; d <= L.reach && i + (size_t)d < M.sites.size() && M.sites[i + (size_t)d].contig == M.sites[i].contig; ++d, ++k) {
            if (k >= lines.size()) return lines;                        // (never: the same walk wrote them)
            if (M.slot(i + (size_t)d)) mark_field(lines[k], 2);
            if (M.slot(i)) mark_field(lines[k], 1);
        }
    return lines;
}

// out_reads and its totals: phase_read_lines's; a block that starts at an insertion site has `+` behind its id
inline bool phase_ins_read_lines(const std::vector<std::string> &contig_names, const std::vector<std::string> &read_names,
                                 const std::vector<uint32_t> &read_of_row, const MergedSites &M, const Blocks &B, const std::vector<ReadRec> &recs,
                                 std::vector<std::string> *lines, ReadTotals *tot) {
    ReadTotals t;
    if (!phase_read_lines(contig_names, read_names, read_of_row, M.sites, B, recs, lines, &t)) return false;
    if (tot) *tot = t;
    if (!lines) return true;
    size_t k = 1;                               // the records that got a line, in order
    for (const ReadRec &r : recs) {
        if ((uint64_t)r.a + r.b + r.other < 1) continue;
        if (k >= lines->size()) return false;
        if (M.slot(B.first[r.block])) mark_field((*lines)[k], 2);
        ++k;
    }
    return k == lines->size();
}

}  // namespace ph
}  // namespace hlmi
