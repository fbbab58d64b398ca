// phase_reach_host_check.cpp - hylight_amd/csrc/phase_reach_text.h (the blocks and phase bits from the links of every distance up
// to `reach`, the bridged sites, the conflict count, the link lines over all distances and the site lines with ".") held to
// literal answers, with the host compiler alone (tests/test_phase_reach_surface.py builds it with -fsanitize=address,undefined
// and runs it).  The answers are the header's rules (include/hylight_mi.h: hlmi_phase_reach) worked by hand;
// tests/test_phase_reach_model.py holds the model to the same hand cases.
#include <cstdio>
#include <string>
#include <vector>

#include "../../hylight_amd/csrc/phase_reach_text.h"

using namespace hlmi::ph;

static int n_bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++n_bad; } \
    } while (0)

static const std::string SITES = "#contig\tpos\tref\talt\tdepth\tref_count\talt_count\tblock\tphase";
static const std::string LINKS = "#contig\tpos1\tpos2\tn00\tn01\tn10\tn11\tinformative\tagree\tphased";
typedef std::vector<std::string> Lines;
typedef std::vector<uint8_t> Bytes;
typedef std::vector<uint32_t> Words;
static const uint8_t X = BIT_BRIDGED;
static const LinkCounts CIS = {3, 0, 0, 3}, TRANS = {0, 3, 3, 0}, TIE = {2, 1, 2, 1}, NONE = {0, 0, 0, 0};

// n sites of contig `contig` on positions 2, 6, 10, ... (own G, alt T, three votes each)
static void add_sites(std::vector<PSite> &s, uint32_t contig, size_t n, uint32_t gbase) {
    for (size_t i = 0; i < n; ++i) s.push_back(PSite{contig, (uint32_t)(2 + 4 * i), gbase + (uint32_t)(2 + 4 * i), 2, 3, {0, 0, 3, 3, 0}});
}
// links of one contig's n sites at reach K: every counter NONE but those given as (j, d, counters)
struct Put {
    size_t j;
    int d;
    LinkCounts c;
};
static ReachLinks links_of(size_t n, int K, const std::vector<Put> &puts) {
    ReachLinks L;
    L.reach = K;
    L.n.assign((n ? n - 1 : 0) * (size_t)K, NONE);
    for (const Put &p : puts) L.n[p.j * (size_t)K + (size_t)(p.d - 1)] = p.c;
    return L;
}

int main() {
    {   // reach 1 is build_blocks: the same call, bit, index and first, the same four counters, on cis - trans - absent - unphased
        std::vector<PSite> sites;
        add_sites(sites, 0, 3, 0);
        add_sites(sites, 2, 2, 12);
        const std::vector<LinkCounts> near = {CIS, TRANS, {9, 9, 9, 9}, {1, 0, 0, 1}};
        ReachLinks L;
        L.reach = 1;
        L.n = near;
        const Blocks B = build_blocks(sites, near, 3, 0.8);
        const ReachBlocks R = build_blocks_reach(sites, L, 3, 0.8);
        EXPECT(R.base.bit == B.bit && R.base.index == B.index && R.base.first == B.first && R.base.call == B.call);
        EXPECT(R.base.links == B.links && R.base.links_phased == B.links_phased && R.base.blocks_multi == B.blocks_multi &&
               R.base.sites_phased == B.sites_phased);
        EXPECT(R.links_far == 0 && R.links_far_phased == 0 && R.joins_far == 0 && R.sites_bridged == 0 && R.links_conflict == 0);
        const Lines names = {"a", "n", "b"};
        EXPECT(phase_reach_site_lines(names, sites, R.base) == phase_site_lines(names, sites, B));
        EXPECT(phase_reach_link_lines(names, sites, L, 3, 0.8) == phase_link_lines(names, sites, near, 3, 0.8));
    }
    {   // a noisy site between two linked ones (tests/phase_reach_inputs.py: noisy_site_between_two_cis / _trans)
        std::vector<PSite> sites;
        add_sites(sites, 0, 3, 0);
        const Lines names = {"c"};
        ReachLinks L = links_of(3, 2, {{0, 1, TIE}, {0, 2, CIS}, {1, 1, {2, 2, 1, 1}}});
        ReachBlocks R = build_blocks_reach(sites, L, 3, 0.8);
        EXPECT((R.base.bit == Bytes{0, X, 0}) && (R.base.index == Words{0, 0, 0}) && (R.base.first == Words{0}));
        EXPECT((R.base.call == Bytes{LINK_UNPHASED, LINK_UNPHASED}) && R.base.links == 2 && R.base.links_phased == 0);
        EXPECT(R.base.blocks_multi == 1 && R.base.sites_phased == 2);
        EXPECT(R.links_far == 1 && R.links_far_phased == 1 && R.joins_far == 1 && R.sites_bridged == 1 && R.links_conflict == 0);
        EXPECT((phase_reach_site_lines(names, sites, R.base) ==
                Lines{SITES, "c\t3\tG\tT\t6\t3\t3\t3\t0|1", "c\t7\tG\tT\t6\t3\t3\t3\t.", "c\t11\tG\tT\t6\t3\t3\t3\t0|1"}));
        EXPECT((phase_reach_link_lines(names, sites, L, 3, 0.8) ==
                Lines{LINKS, "c\t3\t7\t2\t1\t2\t1\t6\t0.500000\t-", "c\t3\t11\t3\t0\t0\t3\t6\t1.000000\tcis", "c\t7\t11\t2\t2\t1\t1\t6\t0.500000\t-"}));
        L = links_of(3, 2, {{0, 1, TIE}, {0, 2, TRANS}, {1, 1, TIE}});
        R = build_blocks_reach(sites, L, 3, 0.8);
        EXPECT((R.base.bit == Bytes{0, X, 1}) && R.joins_far == 1);
        // min_link above the far link's six rows: cut as at reach 1
        R = build_blocks_reach(sites, L, 7, 0.8);
        EXPECT((R.base.bit == Bytes{0, 0, 0}) && (R.base.first == Words{0, 1, 2}) && R.links_far_phased == 0 && R.sites_bridged == 0);
    }
    {   // a pending run of exactly reach sites joins through its last one; of reach + 1 sites it cannot: no such link is read
        std::vector<PSite> sites;
        add_sites(sites, 0, 4, 0);
        ReachBlocks R = build_blocks_reach(sites, links_of(4, 2, {{0, 2, CIS}}), 3, 0.8);
        EXPECT((R.base.bit == Bytes{0, X, 0, 0}) && (R.base.index == Words{0, 0, 0, 1}) && (R.base.first == Words{0, 3}));
        R = build_blocks_reach(sites, links_of(4, 3, {{0, 3, TRANS}}), 3, 0.8);
        EXPECT((R.base.bit == Bytes{0, X, X, 1}) && (R.base.first == Words{0}) && R.sites_bridged == 2 && R.links_far == 3 && R.joins_far == 1);
        // the same counters read at reach 2: entry (0, 3) does not exist; every site a block of one, every bit 0 again
        ReachLinks two = links_of(4, 2, {});
        R = build_blocks_reach(sites, two, 3, 0.8);
        EXPECT((R.base.bit == Bytes{0, 0, 0, 0}) && (R.base.first == Words{0, 1, 2, 3}) && R.sites_bridged == 0 && R.links_far == 2);
        EXPECT(R.base.blocks_multi == 0 && R.base.sites_phased == 0);
        // the pending sites that stay outside start blocks of their own and may join each other: 0 | 1 2 . 4
        add_sites(sites, 0, 1, 16);
        sites[4].pos = sites[4].gpos = 18;
        R = build_blocks_reach(sites, links_of(5, 2, {{1, 1, TRANS}, {2, 2, TRANS}}), 3, 0.8);
        EXPECT((R.base.bit == Bytes{0, 0, 1, X, 0}) && (R.base.index == Words{0, 1, 1, 1, 1}) && (R.base.first == Words{0, 1}));
        EXPECT(R.base.blocks_multi == 1 && R.base.sites_phased == 3 && R.sites_bridged == 1 && R.joins_far == 1);
        // a bridged site is no member: its phased link to a later site joins nothing
        sites.pop_back();
        R = build_blocks_reach(sites, links_of(4, 2, {{0, 2, CIS}, {1, 2, CIS}}), 3, 0.8);
        EXPECT((R.base.bit == Bytes{0, X, 0, 0}) && (R.base.first == Words{0, 3}) && R.links_far_phased == 2);
    }
    {   // the nearest member decides, the far link that says otherwise is counted and changes nothing
        std::vector<PSite> sites;
        add_sites(sites, 0, 3, 0);
        ReachBlocks R = build_blocks_reach(sites, links_of(3, 2, {{0, 1, CIS}, {1, 1, CIS}, {0, 2, TRANS}}), 3, 0.8);
        EXPECT((R.base.bit == Bytes{0, 0, 0}) && R.links_conflict == 1 && R.joins_far == 0 && R.links_far_phased == 1 && R.base.sites_phased == 3);
        R = build_blocks_reach(sites, links_of(3, 2, {{0, 1, CIS}, {1, 1, TRANS}, {0, 2, TRANS}}), 3, 0.8);
        EXPECT((R.base.bit == Bytes{0, 0, 1}) && R.links_conflict == 0);
    }
    {   // a contig junction with fewer than reach sites on either side: no link is counted or written across it, whatever the
        // device left there, and the block ends with the contig
        std::vector<PSite> sites;
        add_sites(sites, 0, 2, 0);
        add_sites(sites, 1, 2, 12);
        ReachLinks L = links_of(4, 3, {{0, 1, CIS}, {0, 2, CIS}, {0, 3, CIS}, {1, 1, CIS}, {1, 2, CIS}, {2, 1, TRANS}});
        const ReachBlocks R = build_blocks_reach(sites, L, 3, 0.8);
        EXPECT((R.base.bit == Bytes{0, 0, 0, 1}) && (R.base.first == Words{0, 2}) && (R.base.call == Bytes{LINK_CIS, LINK_ABSENT, LINK_TRANS}));
        EXPECT(R.base.links == 2 && R.base.links_phased == 2 && R.links_far == 0 && R.links_conflict == 0);
        EXPECT((phase_reach_link_lines({"a", "b"}, sites, L, 3, 0.8) ==
                Lines{LINKS, "a\t3\t7\t3\t0\t0\t3\t6\t1.000000\tcis", "b\t3\t7\t0\t3\t3\t0\t6\t1.000000\ttrans"}));
        // counters that are not there count as zeros
        ReachLinks none;
        none.reach = 8;
        const ReachBlocks E = build_blocks_reach(sites, none, 1, 0.6);
        EXPECT((E.base.first == Words{0, 1, 2, 3}) && E.base.links == 2 && E.links_far == 0);
        EXPECT(phase_reach_link_lines({"a", "b"}, sites, none, 1, 0.6).size() == 3);
    }
    {   // no site, one site
        std::vector<PSite> sites;
        ReachBlocks R = build_blocks_reach(sites, links_of(0, 8, {}), 3, 0.8);
        EXPECT(R.base.first.empty() && R.base.bit.empty() && (phase_reach_site_lines({"c"}, sites, R.base) == Lines{SITES}));
        EXPECT((phase_reach_link_lines({"c"}, sites, links_of(0, 8, {}), 3, 0.8) == Lines{LINKS}));
        add_sites(sites, 0, 1, 0);
        R = build_blocks_reach(sites, links_of(1, 8, {}), 3, 0.8);
        EXPECT((R.base.first == Words{0}) && R.base.call.empty() && R.base.blocks_multi == 0);
    }
    if (n_bad) return 1;
    printf("phase_reach_host_check: ok\n");
    return 0;
}
