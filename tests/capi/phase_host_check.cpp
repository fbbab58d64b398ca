// phase_host_check.cpp - hylight_amd/csrc/phase_text.h (the sites from hlmi_variants's records, the link rule, the blocks and phase
// bits, the hap rule and the lines of the three files of hlmi_phase) held to literal answers, with the host compiler alone
// (tests/test_phase_surface.py builds it with -fsanitize=address,undefined and runs it).  The answers are the header's rules
// (include/hylight_mi.h: hlmi_phase) worked by hand; tests/test_phase_model.py holds the model to the same literals.
#include <cmath>
#include <cstdio>
#include <string>
#include <string_view>
#include <vector>

#include "../../hylight_amd/csrc/phase_text.h"

using namespace hlmi::ph;
using hlmi::var::DeviceVariants;

static int n_bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++n_bad; } \
    } while (0)

static const std::string SITES = "#contig\tpos\tref\talt\tdepth\tref_count\talt_count\tblock\tphase";
static const std::string LINKS = "#contig\tpos1\tpos2\tn00\tn01\tn10\tn11\tinformative\tagree\tphased";
static const std::string READS = "#read\tcontig\tblock\tspanned\thap_a\thap_b\tother\thap";
typedef std::vector<std::string> Lines;

int main() {
    {   // the link rule: cis, trans, a tie, min_link at its border and below, 4 / 5 at 0.8 and at the next double, no row at all
        const LinkCall cis = link_call({3, 0, 0, 3}, 3, 0.8), trans = link_call({0, 3, 3, 0}, 3, 0.8), tie = link_call({1, 1, 1, 1}, 3, 0.8);
        EXPECT(cis.inf == 6 && cis.top == 6 && cis.agree == 1.0 && cis.phased == LINK_CIS);
        EXPECT(trans.inf == 6 && trans.phased == LINK_TRANS);
        EXPECT(tie.inf == 4 && tie.top == 2 && tie.agree == 0.5 && tie.phased == LINK_UNPHASED);
        EXPECT(link_call({3, 0, 0, 3}, 6, 0.8).phased == LINK_CIS && link_call({3, 0, 0, 3}, 7, 0.8).phased == LINK_UNPHASED);
        EXPECT(link_call({2, 0, 1, 2}, 3, 0.8).phased == LINK_CIS && link_call({2, 0, 1, 2}, 3, std::nextafter(0.8, 1.0)).phased == LINK_UNPHASED);
        EXPECT(link_call({1, 2, 2, 0}, 3, 0.8).phased == LINK_TRANS && link_call({1, 2, 2, 0}, 3, 0.8).agree == 0.8);
        const LinkCall none = link_call({0, 0, 0, 0}, 1, 0.6);
        EXPECT(none.inf == 0 && none.agree == 0.0 && none.phased == LINK_UNPHASED);
        EXPECT(link_call({4000000000u, 0, 0, 4000000000u}, 3, 1.0).inf == 8000000000ull);
        EXPECT(hap_of(2, 1) == 'A' && hap_of(1, 2) == 'B' && hap_of(1, 1) == '-' && hap_of(0, 0) == '-');
    }
    {   // contig a (12 bases): sites on positions 2, 6, 10 (own G, G, g) - cis, then trans: bits 0 0 1; contig n without a row;
        // contig b (8 bases) starts at 12 in the device's positions: sites on its positions 0 (own A, alt del) and 7; the link
        // between them has two informative rows: not phased, two blocks.  No link joins a's last site and b's first.
        const Lines names = {"a", "n", "b"}, reads = {"r0", "r1", "r2"};
        const std::vector<std::string_view> seq = {"ACGTACGTACgT", "ACGT", "ACGTACGT"};
        const std::vector<uint32_t> rc = {6, 0, 4}, slot = {0, 0, 1}, cbase = {0, 12, 20};
        DeviceVariants d;
        d.recs = {{2, {0, 0, 3, 3, 0}}, {6, {0, 0, 3, 3, 0}}, {10, {0, 0, 2, 4, 0}}, {12, {2, 0, 0, 0, 2}}, {19, {2, 0, 0, 2, 0}}};
        std::vector<PSite> sites;
        EXPECT(phase_sites(seq, rc, slot, cbase, d, sites) && sites.size() == 5);
        EXPECT(sites[2].contig == 0 && sites[2].pos == 10 && sites[2].own == 2 && sites[2].alt == 3);
        EXPECT(sites[3].contig == 2 && sites[3].pos == 0 && sites[3].gpos == 12 && sites[3].own == 0 && sites[3].alt == 4);
        EXPECT(sites[4].pos == 7 && sites[4].own == 3 && sites[4].alt == 0);
        // the counters of the junction's pair are what the device leaves there: zeros - and were they not, they would not be read
        const std::vector<LinkCounts> links = {{3, 0, 0, 3}, {0, 3, 3, 0}, {9, 9, 9, 9}, {1, 0, 0, 1}};
        const Blocks B = build_blocks(sites, links, 3, 0.8);
        EXPECT((B.bit == std::vector<uint8_t>{0, 0, 1, 0, 0}) && (B.index == std::vector<uint32_t>{0, 0, 0, 1, 2}));
        EXPECT((B.first == std::vector<uint32_t>{0, 3, 4}) && (B.call == std::vector<uint8_t>{LINK_CIS, LINK_TRANS, LINK_ABSENT, LINK_UNPHASED}));
        EXPECT(B.links == 3 && B.links_phased == 2 && B.blocks_multi == 1 && B.sites_phased == 3);
        EXPECT((phase_site_lines(names, sites, B) ==
                Lines{SITES, "a\t3\tG\tT\t6\t3\t3\t3\t0|1", "a\t7\tG\tT\t6\t3\t3\t3\t0|1", "a\t11\tG\tT\t6\t2\t4\t3\t1|0",
                      "b\t1\tA\t*\t4\t2\t2\t1\t0|1", "b\t8\tT\tA\t4\t2\t2\t8\t0|1"}));
        EXPECT((phase_link_lines(names, sites, links, 3, 0.8) ==
                Lines{LINKS, "a\t3\t7\t3\t0\t0\t3\t6\t1.000000\tcis", "a\t7\t11\t0\t3\t3\t0\t6\t1.000000\ttrans", "b\t1\t8\t1\t0\t0\t1\t2\t1.000000\t-"}));
        // row 0 = r2 on a: all three sites, alleles 1 1 0 against bits 0 0 1: hap B; row 1 = r0 on a: a third base alone; row 2 = r1
        // on b: both blocks, a tie of nothing on the first (dropped) and alt on the second
        const std::vector<ReadRec> recs = {{0, 0, 3, 0, 3, 0}, {1, 0, 2, 0, 0, 1}, {2, 1, 1, 0, 0, 0}, {2, 2, 1, 0, 1, 0}};
        const std::vector<uint32_t> read_of_row = {2, 0, 1};
        Lines lines;
        ReadTotals t;
        EXPECT(phase_read_lines(names, reads, read_of_row, sites, B, recs, &lines, &t));
        EXPECT((lines == Lines{READS, "r2\ta\t3\t3\t0\t3\t0\tB", "r0\ta\t3\t2\t0\t0\t1\t-", "r1\tb\t8\t1\t0\t1\t0\tB"}));
        EXPECT(t.records == 3 && t.a == 0 && t.b == 2 && t.tie == 1);
        // the totals alone need no names
        ReadTotals t2;
        EXPECT(phase_read_lines(names, {}, {}, sites, B, recs, nullptr, &t2) && t2.records == 3 && t2.b == 2);
        // a record of a block or of a row that does not exist: refused
        EXPECT(!phase_read_lines(names, reads, read_of_row, sites, B, {{0, 3, 1, 1, 0, 0}}, &lines, nullptr));
        EXPECT(!phase_read_lines(names, reads, read_of_row, sites, B, {{3, 0, 1, 1, 0, 0}}, &lines, nullptr));
        // records on an N, behind the last slot, out of order, without a vote: no sites
        DeviceVariants bad = d;
        bad.recs = {{4, {0, 0, 0, 3, 3}}, {2, {0, 0, 3, 3, 0}}};
        EXPECT(!phase_sites(seq, rc, slot, cbase, bad, sites));
        bad.recs = {{20, {3, 0, 0, 0, 0}}};
        EXPECT(!phase_sites(seq, rc, slot, cbase, bad, sites));
        bad.recs = {{2, {0, 0, 0, 0, 0}}};
        EXPECT(!phase_sites(seq, rc, slot, cbase, bad, sites));
        const std::vector<std::string_view> seq_n = {"ACNTACGTACgT", "ACGT", "ACGTACGT"};
        bad.recs = {{2, {0, 0, 3, 3, 0}}};
        EXPECT(!phase_sites(seq_n, rc, slot, cbase, bad, sites));
    }
    {   // one site: a block of one, no link; no site at all: three header lines
        const Lines names = {"c"};
        const std::vector<std::string_view> seq = {"ACGT"};
        const std::vector<uint32_t> rc = {3}, slot = {0}, cbase = {0, 4};
        DeviceVariants d;
        d.recs = {{1, {2, 1, 0, 0, 0}}};
        std::vector<PSite> sites;
        EXPECT(phase_sites(seq, rc, slot, cbase, d, sites) && sites.size() == 1);
        Blocks B = build_blocks(sites, {}, 3, 0.8);
        EXPECT(B.links == 0 && B.first.size() == 1 && B.blocks_multi == 0 && B.sites_phased == 0 && B.call.empty());
        EXPECT((phase_site_lines(names, sites, B) == Lines{SITES, "c\t2\tC\tA\t3\t1\t2\t2\t0|1"}));
        EXPECT((phase_link_lines(names, sites, {}, 3, 0.8) == Lines{LINKS}));
        d.recs.clear();
        EXPECT(phase_sites(seq, rc, slot, cbase, d, sites) && sites.empty());
        B = build_blocks(sites, {}, 3, 0.8);
        Lines lines;
        ReadTotals t;
        EXPECT(B.first.empty() && (phase_site_lines(names, sites, B) == Lines{SITES}));
        EXPECT(phase_read_lines(names, {}, {}, sites, B, {}, &lines, &t) && lines == Lines{READS} && t.records == 0);
    }
    if (n_bad) return 1;
    printf("phase_host_check: ok\n");
    return 0;
}
