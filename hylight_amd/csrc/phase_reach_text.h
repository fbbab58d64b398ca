// phase_reach_text.h - the host half of hlmi_phase_reach / hlmi_phase_reads_reach (include/hylight_mi.h) that is text and
// arithmetic: the blocks and phase bits from the links of every distance up to `reach`, the bridged sites, the conflict count, the
// link lines over all distances and the site lines with "." for a bridged site.  The link rule, the sites, the hap rule and the
// reads file are phase_text.h's, called and not restated.  Host-only and free of any HIP include, as phase_text.h is:
// tests/capi/phase_reach_host_check.cpp compiles it with the plain host compiler under the sanitizers.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "phase_text.h"

namespace hlmi {
namespace ph {

constexpr int PHASE_REACH_MAX = 8;      // HLMI_PHASE_REACH_MAX
enum : uint8_t { BIT_BRIDGED = 2 };     // a site's `bit` byte beside 0 and 1: inside a block, no member of it

// The counters of the links of every distance as the device writes them: the link (j, j + d), 1 <= d <= reach, is entry
// j * reach + (d - 1); one entry set per site but the last.  An entry whose right site lies on another contig, or behind the last
// site, is never read.
struct ReachLinks {
    int reach = 1;
    std::vector<LinkCounts> n;
    bool has(size_t j, int d) const { return d >= 1 && d <= reach && j * (size_t)reach + (size_t)(d - 1) < n.size(); }
    const LinkCounts &at(size_t j, int d) const { return n[j * (size_t)reach + (size_t)(d - 1)]; }
};

// base: as build_blocks's, with bit[i] == BIT_BRIDGED at a bridged site; call, links and links_phased are about distance 1;
// blocks_multi counts blocks of two or more sites, sites_phased their members
struct ReachBlocks {
    Blocks base;
    uint64_t links_far = 0, links_far_phased = 0, joins_far = 0, sites_bridged = 0, links_conflict = 0;
};

// the call of the link (j, i), j < i <= j + reach, of one contig; counters that are not there count as zeros
inline uint8_t reach_call(const ReachLinks &L, size_t j, size_t i, int min_link, double min_agree) {
    const int d = (int)(i - j);
    return L.has(j, d) ? link_call(L.at(j, d), min_link, min_agree).phased : (uint8_t)LINK_UNPHASED;
}

// The block rule of hlmi_phase_reach.  A block starts at its first site b; site i joins it through the nearest member j,
// i - reach <= j < i, whose link (j, i) is phased, and the walk ends at the first site more than `reach` behind the last member
// or on another contig.  The block is the sites b .. last member; those among them that did not join are bridged.
inline ReachBlocks build_blocks_reach(const std::vector<PSite> &sites, const ReachLinks &L, int min_link, double min_agree) {
    ReachBlocks R;
    Blocks &B = R.base;
    const size_t n = sites.size(), K = (size_t)(L.reach < 1 ? 1 : L.reach);
    B.bit.assign(n, 0);
    B.index.assign(n, 0);
    B.call.assign(n ? n - 1 : 0, LINK_ABSENT);
    auto phased = [](uint8_t c) { return c == LINK_CIS || c == LINK_TRANS; };
    for (size_t i = 0; i + 1 < n; ++i)
        for (size_t d = 1; d <= K && i + d < n && sites[i + d].contig == sites[i].contig; ++d) {
            const uint8_t c = reach_call(L, i, i + d, min_link, min_agree);
            if (d == 1) {
                B.call[i] = c;
                ++B.links;
                B.links_phased += phased(c);
            } else {
                ++R.links_far;
                R.links_far_phased += phased(c);
            }
        }
    for (size_t b = 0; b < n;) {
        size_t last = b, members = 1;
        std::vector<uint8_t> &bit = B.bit;
        bit[b] = 0;
        for (size_t i = b + 1; i < n && i - last <= K && sites[i].contig == sites[b].contig; ++i) {
            bit[i] = BIT_BRIDGED;                                       // until a member in reach says otherwise
            for (size_t j = i; j-- > b && i - j <= K;) {
                if (bit[j] == BIT_BRIDGED) continue;
                const uint8_t c = reach_call(L, j, i, min_link, min_agree);
                if (!phased(c)) continue;
                bit[i] = bit[j] ^ (uint8_t)(c == LINK_TRANS);
                R.joins_far += i - j >= 2;
                last = i;
                ++members;
                break;
            }
        }
        B.first.push_back((uint32_t)b);
        for (size_t i = b; i <= last; ++i) {
            B.index[i] = (uint32_t)B.first.size() - 1;
            R.sites_bridged += bit[i] == BIT_BRIDGED;
        }
        if (last > b) {
            ++B.blocks_multi;
            B.sites_phased += members;
        }
        // a phased link between two members whose direction is not what their bits say: counted, nothing changes
        for (size_t j = b; j < last; ++j)
            for (size_t i = j + 1; i <= last && i - j <= K && bit[j] != BIT_BRIDGED; ++i) {
                if (bit[i] == BIT_BRIDGED) continue;
                const uint8_t c = reach_call(L, j, i, min_link, min_agree);
                R.links_conflict += phased(c) && (uint8_t)(c == LINK_TRANS) != (uint8_t)(bit[j] ^ bit[i]);
            }
        for (size_t i = last + 1; i < n && i - last <= K && sites[i].contig == sites[b].contig; ++i) bit[i] = 0;   // pending sites that stay outside
        b = last + 1;
    }
    return R;
}

// out_sites: phase_site_lines's lines with "." in the phase column of a bridged site
inline std::vector<std::string> phase_reach_site_lines(const std::vector<std::string> &names, const std::vector<PSite> &sites, const Blocks &B) {
    std::vector<std::string> lines;
    lines.reserve(sites.size() + 1);
    lines.push_back("#contig\tpos\tref\talt\tdepth\tref_count\talt_count\tblock\tphase");
    for (size_t i = 0; i < sites.size(); ++i)
        lines.push_back(phase_site_line(names, sites[i], sites[B.first[B.index[i]]], B.bit[i] == BIT_BRIDGED ? "." : B.bit[i] ? "1|0" : "0|1"));
    return lines;
}

// out_links: one line per link of any distance, ordered by (left site, right site)
inline std::vector<std::string> phase_reach_link_lines(const std::vector<std::string> &names, const std::vector<PSite> &sites, const ReachLinks &L,
                                                       int min_link, double min_agree) {
    std::vector<std::string> lines;
    lines.push_back("#contig\tpos1\tpos2\tn00\tn01\tn10\tn11\tinformative\tagree\tphased");
    for (size_t i = 0; i + 1 < sites.size(); ++i)
        for (int d = 1; d <= L.reach && i + (size_t)d < sites.size() && sites[i + (size_t)d].contig == sites[i].contig; ++d)
            lines.push_back(phase_link_line(names, sites[i], sites[i + (size_t)d], L.has(i, d) ? L.at(i, d) : LinkCounts{0, 0, 0, 0}, min_link,
                                            min_agree));
    return lines;
}

}  // namespace ph
}  // namespace hlmi
