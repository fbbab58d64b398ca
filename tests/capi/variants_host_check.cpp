// variants_host_check.cpp - hylight_amd/csrc/variants_text.h (the contig records, the alternative symbol, site_rate, the lines of
// the sites file and of the summary of hlmi_variants) held to literal answers, with the host compiler alone
// (tests/test_variants_surface.py builds it with -fsanitize=address,undefined and runs it).  The answers are the header's rules
// (include/hylight_mi.h: hlmi_variants) worked by hand; tests/test_variants_model.py holds the model to the same literals.
#include <cstdio>
#include <string>
#include <string_view>
#include <vector>

#include "../../hylight_amd/csrc/variants_text.h"

using namespace hlmi::var;

static int n_bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++n_bad; } \
    } while (0)

static const std::string SITES = "#contig\tpos\tref\tdepth\tA\tC\tG\tT\tdel\talt\talt_count\talt_frac";
static const std::string SUMMARY = "#contig\tlength\treads\tcallable\tsites\tsite_rate";
typedef std::vector<std::string> Lines;

int main() {
    {   // the tie rule and the own base
        const uint32_t ac[5] = {2, 2, 1, 0, 0}, td[5] = {1, 0, 0, 2, 2}, none[5] = {5, 0, 0, 0, 0}, del[5] = {3, 0, 0, 0, 2};
        EXPECT(alt_symbol(ac, 2) == 0 && alt_symbol(td, 0) == 3 && alt_symbol(none, 0) == 1 && alt_symbol(del, 0) == 4);
        EXPECT(alt_symbol(ac, 0) == 1);                      // own A: C's two beat G's one
        EXPECT(own_symbol('a') == 0 && own_symbol('C') == 1 && own_symbol('g') == 2 && own_symbol('T') == 3 && own_symbol('N') == -1 &&
               own_symbol('n') == -1 && own_symbol('U') == -1 && own_symbol('*') == -1);
    }
    {   // one contig of 10 bases, sites on positions 2 (own G: A and C tie -> A), 4 (own a, lower case: T and del tie -> T) and 9
        // (own C: del alone)
        const Lines names = {"c"};
        const std::vector<std::string_view> seq = {"ACGTaCGTAC"};
        const std::vector<uint64_t> length = {10};
        const std::vector<uint32_t> rc = {5}, slot = {0}, cbase = {0, 10};
        DeviceVariants d;
        d.callable = {10}; d.ref_other = {0}; d.sites = {3};
        d.recs = {{2, {2, 2, 1, 0, 0}}, {4, {1, 0, 0, 2, 2}}, {9, {0, 3, 0, 0, 2}}};
        VariantTotals t;
        const std::vector<ContigVariants> recs = contig_records(names, length, rc, slot, d, &t);
        Lines lines;
        EXPECT(site_lines(names, seq, rc, slot, cbase, d, lines, &t));
        EXPECT(t.contigs_covered == 1 && t.positions == 10 && t.callable == 10 && t.sites == 3 && t.sites_base == 2 && t.sites_del == 1);
        EXPECT((lines == Lines{SITES, "c\t3\tG\t5\t2\t2\t1\t0\t0\tA\t2\t0.400000", "c\t5\tA\t5\t1\t0\t0\t2\t2\tT\t2\t0.400000",
                               "c\t10\tC\t5\t0\t3\t0\t0\t2\t*\t2\t0.400000"}));
        EXPECT((summary_lines(recs) == Lines{SUMMARY, "c\t10\t5\t10\t3\t0.300000"}));
    }
    {   // a (8 bases), n (6 bases, no row), e (no bases), b (10 bases): the records of a and b lie side by side in the device's
        // positions (b starts at 8): the last position of a and the first of b are both sites; b has an N (ref_other) and 1 / 3
        const Lines names = {"a", "n", "e", "b"};
        const std::vector<std::string_view> seq = {"ACGTACGT", "ACGTAC", "", "GNACGTACGT"};
        const std::vector<uint64_t> length = {8, 6, 0, 10};
        const std::vector<uint32_t> rc = {2, 0, 0, 7}, slot = {0, 0, 0, 1}, cbase = {0, 8, 18};
        DeviceVariants d;
        d.callable = {8, 3}; d.ref_other = {0, 1}; d.sites = {1, 1};
        d.recs = {{7, {0, 0, 0, 4, 1}}, {8, {1, 0, 6, 0, 0}}};
        VariantTotals t;
        const std::vector<ContigVariants> recs = contig_records(names, length, rc, slot, d, &t);
        Lines lines;
        EXPECT(site_lines(names, seq, rc, slot, cbase, d, lines, &t));
        EXPECT(t.contigs_covered == 2 && t.positions == 24 && t.callable == 11 && t.ref_other == 1 && t.sites == 2 && t.sites_base == 1 &&
               t.sites_del == 1);
        EXPECT((lines == Lines{SITES, "a\t8\tT\t5\t0\t0\t0\t4\t1\t*\t1\t0.200000", "b\t1\tG\t7\t1\t0\t6\t0\t0\tA\t1\t0.142857"}));
        EXPECT((summary_lines(recs) == Lines{SUMMARY, "a\t8\t2\t8\t1\t0.125000", "n\t6\t0\t0\t0\t0.000000", "e\t0\t0\t0\t0\t0.000000",
                                             "b\t10\t7\t3\t1\t0.333333"}));
        // a record on the N, one behind the last slot, one in front of its slot's turn: refused, not written
        DeviceVariants bad = d;
        bad.recs = {{9, {3, 0, 0, 0, 0}}};
        EXPECT(!site_lines(names, seq, rc, slot, cbase, bad, lines, nullptr));
        bad.recs = {{18, {3, 0, 0, 0, 0}}};
        EXPECT(!site_lines(names, seq, rc, slot, cbase, bad, lines, nullptr));
        bad.recs = {{8, {1, 0, 6, 0, 0}}, {7, {0, 0, 0, 4, 1}}};
        EXPECT(!site_lines(names, seq, rc, slot, cbase, bad, lines, nullptr));
        bad.recs = {{7, {0, 0, 0, 0, 0}}};
        EXPECT(!site_lines(names, seq, rc, slot, cbase, bad, lines, nullptr));
    }
    {   // nothing selected anywhere: the header line alone, a summary of zeros; no device output at all
        const Lines names = {"e", "c"};
        const std::vector<std::string_view> seq = {"", "ACGT"};
        const std::vector<uint64_t> length = {0, 4};
        const std::vector<uint32_t> rc = {0, 0}, slot = {0, 0}, cbase = {0};
        const DeviceVariants d;
        VariantTotals t;
        const std::vector<ContigVariants> recs = contig_records(names, length, rc, slot, d, &t);
        Lines lines;
        EXPECT(site_lines(names, seq, rc, slot, cbase, d, lines, &t) && lines == Lines{SITES});
        EXPECT(t.contigs_covered == 0 && t.positions == 4 && t.callable == 0 && t.sites == 0);
        EXPECT((summary_lines(recs) == Lines{SUMMARY, "e\t0\t0\t0\t0\t0.000000", "c\t4\t0\t0\t0\t0.000000"}));
    }
    {   // no contig at all
        const DeviceVariants d;
        Lines lines;
        EXPECT(site_lines({}, {}, {}, {}, {0}, d, lines, nullptr) && lines == Lines{SITES});
        EXPECT((summary_lines(contig_records({}, {}, {}, {}, d, nullptr)) == Lines{SUMMARY}));
    }
    if (n_bad) return 1;
    printf("variants_host_check: ok\n");
    return 0;
}
